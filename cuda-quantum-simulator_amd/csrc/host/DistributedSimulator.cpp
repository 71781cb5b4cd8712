// DistributedSimulator.cpp — Simulator's interface on the sharded engine, over the C ABI
// (qsim_dist_*).
#include "qsim/DistributedSimulator.hpp"

#include <stdexcept>
#include <string>
#include <utility>

#include "abi_util.hpp"

namespace qsim {

using detail::check;

DistributedSimulator::DistributedSimulator(int num_qubits, int rank, int world, const UniqueId& unique_id,
                                           int device)
    : num_qubits_(num_qubits), rank_(rank), world_(world) {
    static_assert(sizeof(UniqueId) == QSIM_DIST_UNIQUE_ID_BYTES, "unique id size");
    check(qsim_dist_create(num_qubits, rank, world, unique_id.data(), device, &h_));
}

DistributedSimulator::~DistributedSimulator() {
    if (h_) (void)qsim_dist_destroy(h_);
}

DistributedSimulator::DistributedSimulator(DistributedSimulator&& o) noexcept
    : h_(o.h_), num_qubits_(o.num_qubits_), rank_(o.rank_), world_(o.world_), virtual_(o.virtual_),
      mode_(o.mode_), seeded_(o.seeded_), rng_(o.rng_) {
    o.h_ = nullptr;
}

DistributedSimulator& DistributedSimulator::operator=(DistributedSimulator&& o) noexcept {
    if (this != &o) {
        if (h_) (void)qsim_dist_destroy(h_);
        h_ = o.h_;
        num_qubits_ = o.num_qubits_;
        rank_ = o.rank_;
        world_ = o.world_;
        virtual_ = o.virtual_;
        mode_ = o.mode_;
        seeded_ = o.seeded_;
        rng_ = o.rng_;
        o.h_ = nullptr;
    }
    return *this;
}

DistributedSimulator::UniqueId DistributedSimulator::uniqueId() {
    UniqueId id{};
    check(qsim_dist_unique_id(id.data()));
    return id;
}

DistributedSimulator DistributedSimulator::makeVirtual(int num_qubits, int world, int device) {
    DistributedSimulator s;
    s.num_qubits_ = num_qubits;
    s.world_ = world;
    s.virtual_ = true;
    check(qsim_dist_create_virtual(num_qubits, world, device, &s.h_));
    return s;
}

void DistributedSimulator::reset() { check(qsim_dist_reset(h_)); }

void DistributedSimulator::run(const Circuit& circuit) {
    if (circuit.getNumQubits() != num_qubits_)
        throw std::invalid_argument("Circuit qubit count doesn't match simulator");
    const std::vector<qsim_gate> gates = detail::toAbi(circuit);
    check(qsim_dist_run(h_, gates.data(), gates.size(),
                        mode_ == RunMode::Fused ? QSIM_RUN_FUSED : QSIM_RUN_PER_GATE));
}

void DistributedSimulator::runSequence(const std::vector<Circuit>& circuits) {
    std::vector<qsim_gate> gates;
    for (const Circuit& c : circuits) {
        if (c.getNumQubits() != num_qubits_)
            throw std::invalid_argument("Circuit qubit count doesn't match simulator");
        const std::vector<qsim_gate> g = detail::toAbi(c);
        gates.insert(gates.end(), g.begin(), g.end());
    }
    check(qsim_dist_run(h_, gates.data(), gates.size(),
                        mode_ == RunMode::Fused ? QSIM_RUN_FUSED : QSIM_RUN_PER_GATE));
}

std::vector<std::complex<double>> DistributedSimulator::getStateVector() const {
    std::vector<std::complex<double>> out(root() ? (size_t)1 << num_qubits_ : 0);
    check(qsim_dist_gather_state(h_, root() ? reinterpret_cast<double*>(out.data()) : nullptr));
    return out;
}

std::vector<double> DistributedSimulator::getProbabilities() const {
    std::vector<double> out(root() ? (size_t)1 << num_qubits_ : 0);
    check(qsim_dist_probabilities(h_, root() ? out.data() : nullptr));
    return out;
}

double DistributedSimulator::expectation(const PauliSum& observable) const {
    if (observable.getNumQubits() != num_qubits_)
        throw std::invalid_argument("Observable qubit count doesn't match simulator");
    std::vector<qsim_pauli_term> terms;
    terms.reserve(observable.size());
    for (const PauliSum::Term& t : observable.terms()) terms.push_back(qsim_pauli_term{t.x_mask, t.z_mask, t.coeff});
    double e = 0.0;
    check(qsim_dist_expectation(h_, terms.data(), terms.size(), &e));
    return e;
}

std::vector<double> DistributedSimulator::marginalProbabilities(const std::vector<int>& qubits) const {
    if (qubits.size() > 20) throw std::invalid_argument("at most 20 qubits in a marginal");
    std::vector<double> out(size_t(1) << qubits.size());
    check(qsim_dist_marginal_probabilities(h_, qubits.data(), (int)qubits.size(), out.data()));
    return out;
}

std::vector<std::complex<double>> DistributedSimulator::reducedDensityMatrix(const std::vector<int>& qubits) const {
    if (qubits.size() > 6) throw std::invalid_argument("at most 6 qubits in a reduced density matrix");
    std::vector<std::complex<double>> out(size_t(1) << (2 * qubits.size()));
    // std::complex<double> is layout-compatible with double[2] ([complex.numbers.general]).
    check(qsim_dist_reduced_density_matrix(h_, qubits.data(), (int)qubits.size(),
                                           reinterpret_cast<double*>(out.data())));
    return out;
}

double DistributedSimulator::subsystemPurity(const std::vector<int>& qubits) const {
    double tr2 = 0.0;
    for (const auto& v : reducedDensityMatrix(qubits)) tr2 += std::norm(v);
    return tr2;
}

double DistributedSimulator::entanglementEntropy(const std::vector<int>& qubits, bool renyi2) const {
    return hermitianEntropy(reducedDensityMatrix(qubits), 1 << qubits.size(), renyi2);
}

Gradient DistributedSimulator::gradient(const Circuit& circuit, const PauliSum& observable, RunMode mode) {
    if (circuit.getNumQubits() != num_qubits_)
        throw std::invalid_argument("Circuit qubit count doesn't match simulator");
    if (observable.getNumQubits() != num_qubits_)
        throw std::invalid_argument("Observable qubit count doesn't match simulator");
    const std::vector<qsim_gate> gates = detail::toAbi(circuit);
    std::vector<qsim_pauli_term> terms;
    terms.reserve(observable.size());
    for (const PauliSum::Term& t : observable.terms()) terms.push_back(qsim_pauli_term{t.x_mask, t.z_mask, t.coeff});
    Gradient out{0.0, std::vector<double>(gates.size(), 0.0)};
    check(qsim_dist_gradient(h_, gates.data(), gates.size(), terms.data(), terms.size(),
                             mode == RunMode::Fused ? QSIM_RUN_FUSED : QSIM_RUN_PER_GATE, &out.value,
                             out.gradient.data()));
    return out;
}

void DistributedSimulator::releaseGradientBuffers() {
    check(qsim_dist_gradient_release(h_));
}

namespace {
std::vector<qsim_pauli_term> termsOf(const PauliSum& p, int n, const char* what) {
    if (p.getNumQubits() != n) throw std::invalid_argument(std::string(what) + " qubit count doesn't match simulator");
    std::vector<qsim_pauli_term> out;
    out.reserve(p.size());
    for (const PauliSum::Term& t : p.terms()) out.push_back(qsim_pauli_term{t.x_mask, t.z_mask, t.coeff});
    return out;
}
}  // namespace

void DistributedSimulator::applyPauliRotation(const std::vector<std::pair<int, char>>& factors, double theta) {
    applyPauliRotations(PauliSum(num_qubits_).add(theta, factors));
}

void DistributedSimulator::applyPauliRotations(const PauliSum& seq) {
    const std::vector<qsim_pauli_term> rots = termsOf(seq, num_qubits_, "Rotation sequence");
    check(qsim_dist_apply_pauli_rotations(h_, rots.data(), rots.size()));
}

void DistributedSimulator::evolve(const PauliSum& H, double time, int steps, int order) {
    applyPauliRotations(trotter_sequence(H, time, steps, order));
}

Gradient DistributedSimulator::pauliGradient(const PauliSum& seq, const PauliSum& observable) {
    const std::vector<qsim_pauli_term> rots = termsOf(seq, num_qubits_, "Rotation sequence");
    const std::vector<qsim_pauli_term> terms = termsOf(observable, num_qubits_, "Observable");
    Gradient g{0.0, std::vector<double>(rots.size(), 0.0)};
    check(qsim_dist_pauli_gradient(h_, rots.data(), rots.size(), terms.data(), terms.size(), &g.value,
                                   g.gradient.data()));
    return g;
}

void DistributedSimulator::setSeed(unsigned int seed) {
    rng_.seed(seed);
    seeded_ = true;
}

// Rank 0's draws, on every rank (StateVector::uniforms, then the broadcast).
std::vector<double> DistributedSimulator::uniforms(int count) {
    std::uniform_real_distribution<double> dist(0.0, 1.0);
    std::vector<double> u(count);
    if (seeded_) {
        for (double& x : u) x = dist(rng_);
    } else {
        std::random_device rd;
        std::mt19937 rng(rd());
        for (double& x : u) x = dist(rng);
    }
    check(qsim_dist_bcast(h_, u.data(), u.size()));
    return u;
}

std::vector<int> DistributedSimulator::sample(int n_shots) {
    if (n_shots == 0) return {};
    if (n_shots < 0) throw std::invalid_argument("n_shots must be positive");
    const std::vector<double> u = uniforms(n_shots);
    std::vector<int64_t> idx(n_shots);
    check(qsim_dist_sample(h_, u.data(), n_shots, idx.data()));
    return std::vector<int>(idx.begin(), idx.end());
}

int DistributedSimulator::measureQubit(int qubit) {
    if (qubit < 0 || qubit >= num_qubits_)
        throw std::invalid_argument("Qubit index " + std::to_string(qubit) + " out of range [0, " +
                                    std::to_string(num_qubits_ - 1) + "]");
    const double u = uniforms(1)[0];
    int result = 0;
    check(qsim_dist_measure(h_, num_qubits_ - 1 - qubit, u, &result));
    return result;
}

void DistributedSimulator::synchronize() const { check(qsim_dist_sync(h_)); }

}  // namespace qsim
