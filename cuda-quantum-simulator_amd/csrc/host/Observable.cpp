// Observable.cpp — PauliSum and the expectation-value methods of the simulators over the C ABI
// (qsim_state_expectation / qsim_batch_expectation).  No reference counterpart.
#include "qsim/Observable.hpp"

#include <stdexcept>
#include <string>

#include "abi_util.hpp"
#include "qsim/NoiseModel.hpp"
#include "qsim/Simulator.hpp"
#include "qsim/StateVector.hpp"
#include "qsim_circuits.h"

namespace qsim {

using detail::check;

PauliSum::PauliSum(int num_qubits) : num_qubits_(num_qubits) {
    if (num_qubits < QSIM_MIN_QUBITS || num_qubits > QSIM_MAX_QUBITS_SINGLE)
        throw std::invalid_argument("Number of qubits must be between 1 and 30");
}

PauliSum& PauliSum::add(double coeff, const std::vector<std::pair<int, char>>& factors) {
    Term t{0, 0, coeff};
    uint64_t seen = 0;
    for (const auto& f : factors) {
        const int q = f.first;
        if (q < 0 || q >= num_qubits_)
            throw std::out_of_range("Qubit index " + std::to_string(q) + " out of range");
        const uint64_t bit = 1ull << q;
        if (seen & bit) throw std::invalid_argument("Qubit " + std::to_string(q) + " repeated in a Pauli term");
        seen |= bit;
        switch (f.second) {
            case 'X': t.x_mask |= bit; break;
            case 'Y': t.x_mask |= bit; t.z_mask |= bit; break;
            case 'Z': t.z_mask |= bit; break;
            default: throw std::invalid_argument(std::string("Unknown Pauli letter '") + f.second + "'");
        }
    }
    terms_.push_back(t);
    return *this;
}

PauliSum trotter_sequence(const PauliSum& H, double time, int steps, int order) {
    if (steps < 1) throw std::invalid_argument("steps must be at least 1");
    if (order != 1 && order != 2) throw std::invalid_argument("order must be 1 or 2");
    PauliSum seq(H.getNumQubits());
    const std::vector<PauliSum::Term>& terms = H.terms();
    const size_t T = terms.size();
    auto rot = [&](size_t t, double scale) {
        seq.terms_.push_back(
            PauliSum::Term{terms[t].x_mask, terms[t].z_mask, scale * (2.0 * terms[t].coeff * time / steps)});
    };
    if (order == 1 || T <= 1) {
        for (int s = 0; s < steps; ++s)
            for (size_t t = 0; t < T; ++t) rot(t, 1.0);
        return seq;
    }
    for (int s = 0; s < steps; ++s) {
        rot(0, s == 0 ? 0.5 : 1.0);  // (step s - 1 ended with the other half)
        for (size_t t = 1; t + 1 < T; ++t) rot(t, 0.5);
        rot(T - 1, 1.0);
        for (size_t t = T - 1; t-- > 1;) rot(t, 0.5);
    }
    rot(0, 0.5);
    return seq;
}

static std::vector<qsim_pauli_term> toAbi(const PauliSum& p, int num_qubits) {
    if (p.getNumQubits() != num_qubits)
        throw std::invalid_argument("Observable qubit count doesn't match simulator");
    std::vector<qsim_pauli_term> v;
    v.reserve(p.size());
    for (const PauliSum::Term& t : p.terms()) v.push_back(qsim_pauli_term{t.x_mask, t.z_mask, t.coeff});
    return v;
}

double StateVector::expectation(const PauliSum& observable) const {
    const std::vector<qsim_pauli_term> terms = toAbi(observable, num_qubits_);
    double e = 0.0;
    check(qsim_state_expectation(h_, terms.data(), terms.size(), &e));
    return e;
}

double Simulator::expectation(const PauliSum& observable) const { return state_.expectation(observable); }

void StateVector::applyPauliSum(const PauliSum& observable, StateVector& dst) const {
    const std::vector<qsim_pauli_term> terms = toAbi(observable, num_qubits_);
    check(qsim_state_apply_pauli_sum(h_, dst.h_, terms.data(), terms.size()));
}

std::complex<double> StateVector::innerProduct(const StateVector& other) const {
    double out[2] = {0.0, 0.0};
    check(qsim_state_inner_product(h_, other.h_, out));
    return {out[0], out[1]};
}

Gradient Simulator::gradient(const Circuit& circuit, const PauliSum& observable, RunMode mode) {
    if (circuit.getNumQubits() != state_.getNumQubits())
        throw std::invalid_argument("Circuit qubit count doesn't match simulator");
    const std::vector<qsim_pauli_term> terms = toAbi(observable, state_.getNumQubits());
    const std::vector<qsim_gate> gates = detail::toAbi(circuit);
    Gradient g{0.0, std::vector<double>(gates.size(), 0.0)};
    check(qsim_state_gradient(state_.handle(), gates.data(), gates.size(), terms.data(), terms.size(),
                              mode == RunMode::Fused ? QSIM_RUN_FUSED : QSIM_RUN_PER_GATE, &g.value,
                              g.gradient.data()));
    return g;
}

void StateVector::applyPauliRotation(const std::vector<std::pair<int, char>>& factors, double theta) {
    applyPauliRotations(PauliSum(num_qubits_).add(theta, factors));
}

void StateVector::applyPauliRotations(const PauliSum& seq) {
    const std::vector<qsim_pauli_term> rots = toAbi(seq, num_qubits_);
    check(qsim_state_apply_pauli_rotations(h_, rots.data(), rots.size()));
}

void Simulator::applyPauliRotation(const std::vector<std::pair<int, char>>& factors, double theta) {
    state_.applyPauliRotation(factors, theta);
}

void Simulator::applyPauliRotations(const PauliSum& seq) { state_.applyPauliRotations(seq); }

void Simulator::evolve(const PauliSum& H, double time, int steps, int order) {
    state_.applyPauliRotations(trotter_sequence(H, time, steps, order));
}

Gradient Simulator::pauliGradient(const PauliSum& seq, const PauliSum& observable) {
    const std::vector<qsim_pauli_term> rots = toAbi(seq, state_.getNumQubits());
    const std::vector<qsim_pauli_term> terms = toAbi(observable, state_.getNumQubits());
    Gradient g{0.0, std::vector<double>(rots.size(), 0.0)};
    check(qsim_state_pauli_gradient(state_.handle(), rots.data(), rots.size(), terms.data(), terms.size(), &g.value,
                                    g.gradient.data()));
    return g;
}

void Simulator::releaseGradientBuffers() { check(qsim_state_gradient_release(state_.handle())); }

double NoisySimulator::expectation(const PauliSum& observable) const { return state_.expectation(observable); }

std::vector<double> BatchedSimulator::getExpectations(const PauliSum& observable) {
    const std::vector<qsim_pauli_term> terms = toAbi(observable, num_qubits_);
    std::vector<double> e((size_t)batch_size_);
    check(qsim_batch_expectation(h_, terms.data(), terms.size(), e.data()));
    return e;
}

double BatchedSimulator::getAverageExpectation(const PauliSum& observable) {
    const std::vector<double> e = getExpectations(observable);
    double sum = 0.0;
    for (double v : e) sum += v;
    return sum / (double)e.size();
}

}  // namespace qsim

extern "C" int qsim_pauli_term_make(int n_qubits, const int32_t* qubits, const char* letters, size_t count,
                                    double coeff, qsim_pauli_term* out) {
    try {
        if (!out || (count && (!qubits || !letters))) throw std::invalid_argument("null buffer");
        qsim::PauliSum p(n_qubits);
        std::vector<std::pair<int, char>> factors;
        for (size_t i = 0; i < count; ++i) factors.emplace_back(qubits[i], letters[i]);
        p.add(coeff, factors);
        *out = qsim_pauli_term{p.terms()[0].x_mask, p.terms()[0].z_mask, p.terms()[0].coeff};
        return QSIM_OK;
    } catch (const std::invalid_argument&) {
        return QSIM_ERR_INVALID_ARGUMENT;
    } catch (const std::out_of_range&) {
        return QSIM_ERR_OUT_OF_RANGE;
    } catch (const std::exception&) {
        return QSIM_ERR_RUNTIME;
    }
}
