// Marginal.cpp — marginal probabilities, reduced density matrices, subsystem purity and
// entanglement entropy of the simulators over the C ABI (qsim_state_marginal_probabilities /
// qsim_state_reduced_density_matrix), and the host eigenvalue routine behind the entropy.  No
// reference counterpart.
#include <algorithm>
#include <cmath>
#include <complex>
#include <stdexcept>
#include <vector>

#include "abi_util.hpp"
#include "qsim/NoiseModel.hpp"
#include "qsim/Simulator.hpp"
#include "qsim/StateVector.hpp"
#include "qsim_circuits.h"

namespace qsim {

using detail::check;

// Eigenvalues of a Hermitian dim x dim matrix (row-major) by cyclic Jacobi sweeps: every
// off-diagonal element a_pq in turn is zeroed by the unitary plane rotation
//     J = [[c, -s e^{i phi}], [s e^{-i phi}, c]],  phi = arg a_pq,  tan(2 theta) = 2 |a_pq| / (a_pp - a_qq)
// taken with |theta| <= pi/4, until the off-diagonal mass is at rounding level.
std::vector<double> hermitianEigenvalues(std::vector<std::complex<double>> a, int dim) {
    using cd = std::complex<double>;
    if (dim < 1 || a.size() != (size_t)dim * dim) throw std::invalid_argument("matrix must be dim x dim");
    auto at = [&](int r, int c) -> cd& { return a[(size_t)r * dim + c]; };
    double scale = 0.0;
    for (const cd& v : a) scale = std::max(scale, std::abs(v));
    for (int sweep = 0; sweep < 64 && scale > 0.0; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < dim; ++p)
            for (int q = p + 1; q < dim; ++q) off += std::norm(at(p, q));
        if (std::sqrt(off) <= 1e-18 * scale * dim) break;
        for (int p = 0; p < dim; ++p)
            for (int q = p + 1; q < dim; ++q) {
                const cd apq = at(p, q);
                const double g = std::abs(apq);
                if (g == 0.0) continue;
                const double app = at(p, p).real(), aqq = at(q, q).real();
                const cd ph = apq / g;  // e^{i phi}
                const double tau = (aqq - app) / (2.0 * g);
                const double t = (tau >= 0.0 ? 1.0 : -1.0) / (std::abs(tau) + std::sqrt(1.0 + tau * tau));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
                // A <- J^dagger A J with J = [[c, s ph], [-s conj(ph), c]] on the (p, q) plane
                for (int r = 0; r < dim; ++r) {  // columns p, q
                    const cd xp = at(r, p), xq = at(r, q);
                    at(r, p) = c * xp - s * std::conj(ph) * xq;
                    at(r, q) = s * ph * xp + c * xq;
                }
                for (int r = 0; r < dim; ++r) {  // rows p, q
                    const cd xp = at(p, r), xq = at(q, r);
                    at(p, r) = c * xp - s * ph * xq;
                    at(q, r) = s * std::conj(ph) * xp + c * xq;
                }
                at(p, q) = at(q, p) = cd(0.0, 0.0);
                at(p, p) = cd(at(p, p).real(), 0.0);
                at(q, q) = cd(at(q, q).real(), 0.0);
            }
    }
    std::vector<double> ev(dim);
    for (int i = 0; i < dim; ++i) ev[i] = at(i, i).real();
    std::sort(ev.begin(), ev.end());
    return ev;
}

double hermitianEntropy(const std::vector<std::complex<double>>& rho, int dim, bool renyi2) {
    if (dim < 1 || rho.size() != (size_t)dim * dim) throw std::invalid_argument("matrix must be dim x dim");
    if (renyi2) {
        double tr2 = 0.0;  // Tr rho^2 = sum |rho_ij|^2 for a Hermitian rho
        for (const auto& v : rho) tr2 += std::norm(v);
        return -std::log2(tr2);
    }
    double h = 0.0;
    for (double l : hermitianEigenvalues(rho, dim))
        if (l >= 1e-300) h -= l * std::log2(l);
    return h;
}

std::vector<double> StateVector::marginalProbabilities(const std::vector<int>& qubits) const {
    if (qubits.size() > 20) throw std::invalid_argument("at most 20 qubits in a marginal");
    std::vector<double> out(size_t(1) << qubits.size());
    check(qsim_state_marginal_probabilities(h_, qubits.data(), (int)qubits.size(), out.data()));
    return out;
}

std::vector<std::complex<double>> StateVector::reducedDensityMatrix(const std::vector<int>& qubits) const {
    if (qubits.size() > 6) throw std::invalid_argument("at most 6 qubits in a reduced density matrix");
    std::vector<std::complex<double>> out(size_t(1) << (2 * qubits.size()));
    // std::complex<double> is layout-compatible with double[2] ([complex.numbers.general]).
    check(qsim_state_reduced_density_matrix(h_, qubits.data(), (int)qubits.size(),
                                            reinterpret_cast<double*>(out.data())));
    return out;
}

double StateVector::subsystemPurity(const std::vector<int>& qubits) const {
    double tr2 = 0.0;
    for (const auto& v : reducedDensityMatrix(qubits)) tr2 += std::norm(v);
    return tr2;
}

double StateVector::entanglementEntropy(const std::vector<int>& qubits, bool renyi2) const {
    return hermitianEntropy(reducedDensityMatrix(qubits), 1 << qubits.size(), renyi2);
}

std::vector<double> Simulator::marginalProbabilities(const std::vector<int>& q) const { return state_.marginalProbabilities(q); }
std::vector<std::complex<double>> Simulator::reducedDensityMatrix(const std::vector<int>& q) const { return state_.reducedDensityMatrix(q); }
double Simulator::subsystemPurity(const std::vector<int>& q) const { return state_.subsystemPurity(q); }
double Simulator::entanglementEntropy(const std::vector<int>& q, bool renyi2) const { return state_.entanglementEntropy(q, renyi2); }

std::vector<double> NoisySimulator::marginalProbabilities(const std::vector<int>& q) const { return state_.marginalProbabilities(q); }
std::vector<std::complex<double>> NoisySimulator::reducedDensityMatrix(const std::vector<int>& q) const { return state_.reducedDensityMatrix(q); }
double NoisySimulator::subsystemPurity(const std::vector<int>& q) const { return state_.subsystemPurity(q); }
double NoisySimulator::entanglementEntropy(const std::vector<int>& q, bool renyi2) const { return state_.entanglementEntropy(q, renyi2); }

}  // namespace qsim

extern "C" int qsim_hermitian_entropy(const double* rho, int dim, int renyi2, double* out) {
    if (!rho || !out || dim < 1 || dim > 64) return QSIM_ERR_INVALID_ARGUMENT;
    try {
        std::vector<std::complex<double>> m((size_t)dim * dim);
        for (size_t i = 0; i < m.size(); ++i) m[i] = {rho[2 * i], rho[2 * i + 1]};
        *out = qsim::hermitianEntropy(m, dim, renyi2 != 0);
        return QSIM_OK;
    } catch (const std::exception&) {
        return QSIM_ERR_RUNTIME;
    }
}
