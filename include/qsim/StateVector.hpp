// StateVector.hpp — GPU-resident 2^n complex<double> state (reference include/StateVector.cuh:66-124).
//
// Host-only header: the device buffer and its HIP stream live behind the C ABI handle
// qsim_state (include/qsim_hip.h).  Move-only RAII owner like the reference (copy deleted,
// moved-from object holds nothing: src/StateVector.cu:150-171).
#pragma once

#include <complex>
#include <cstddef>
#include <cstdint>
#include <random>
#include <utility>
#include <vector>

struct qsim_state;

namespace qsim {

class PauliSum;  // Observable.hpp

// Layout of one device amplitude: interleaved {re, im} doubles (what devicePtr() points at).
struct Amplitude {
    double re;
    double im;
};

class StateVector {
public:
    explicit StateVector(int num_qubits);  // std::invalid_argument outside [1, 30]
    ~StateVector();
    StateVector(const StateVector&) = delete;
    StateVector& operator=(const StateVector&) = delete;
    StateVector(StateVector&& other) noexcept;
    StateVector& operator=(StateVector&& other) noexcept;

    void initializeZero();
    void initializeBasis(size_t basis_idx);  // std::invalid_argument if >= 2^n

    int getNumQubits() const { return num_qubits_; }
    size_t getSize() const { return size_; }

    // Device address of amplitude 0 (for the kernel-level entry qsim_apply_gate_raw).
    Amplitude* devicePtr();
    const Amplitude* devicePtr() const;

    // General controlled 2x2 unitary [[m0, m1], [m2, m3]] on `target` (src/OptimizedGates.cu:165-183
    // applyGate1Q_coalesced, plus controls); std::out_of_range / std::invalid_argument on bad qubits.
    void applyMatrix1Q(int target, const std::complex<double> (&m)[4],
                       const std::vector<int>& controls = {});
    // General 2^k x 2^k matrix (row-major, k = targets.size() <= 8; matrix-index bit j = qubit
    // targets[j]) on the control == 1 subspace (qsim_apply_matrix).
    void applyMatrix(const std::vector<int>& targets, const std::vector<std::complex<double>>& m,
                     const std::vector<int>& controls = {});

    std::vector<std::complex<double>> toHost() const;
    void fromHost(const std::vector<std::complex<double>>& amplitudes);
    std::vector<double> getProbabilities() const;
    double getTotalProbability() const;  // device wave64 reduction
    bool isNormalized(double tolerance = 1e-10) const;
    // Extensions (no reference counterpart): the larger per-component |a - b| against another
    // state of the same size, on the device; the device bytes this state owns now
    // (qsim_state_max_abs_diff / qsim_state_memory_bytes).
    double maxAbsDiff(const StateVector& other) const;
    size_t getDeviceMemoryBytes() const;
    // <psi|H|psi> of a Pauli sum (Observable.hpp), reduced on the device where the state lies:
    // no readback and no layout restore (qsim_state_expectation).  No reference counterpart.
    // std::invalid_argument on a qubit-count mismatch.
    double expectation(const PauliSum& observable) const;
    // dst = H |this> out of place on the device (qsim_state_apply_pauli_sum); dst takes this
    // state's qubit layout.  std::invalid_argument on a qubit-count mismatch or &dst == this.
    void applyPauliSum(const PauliSum& observable, StateVector& dst) const;
    // exp(-i theta/2 P) in place, P the product of the factors (qubit, 'X' | 'Y' | 'Z') (none: the
    // global phase exp(-i theta/2)): one streaming pass over the state whatever the string's
    // weight.  std::out_of_range on a bad qubit, before anything is applied.
    void applyPauliRotation(const std::vector<std::pair<int, char>>& factors, double theta);
    // A PauliSum read as an ordered sequence: term t is exp(-i coeff_t/2 P_t), applied in add()
    // order where the state lies, no layout restore (qsim_state_apply_pauli_rotations; no reference
    // counterpart).  A run of consecutive Z/I-only rotations shares one pass.  Asynchronous.
    // std::invalid_argument on a qubit-count mismatch.
    void applyPauliRotations(const PauliSum& seq);
    // <this|other> by a fixed-order device reduction (qsim_state_inner_product): bitwise
    // reproducible; innerProduct(*this) is the norm.  std::invalid_argument on a size mismatch.
    std::complex<double> innerProduct(const StateVector& other) const;
    void assertNormalized(double tolerance = 1e-10) const;  // std::runtime_error

    // Readout of a subset of qubits where the state lies: one streaming read, no readback of the
    // amplitudes, no layout restore (qsim_state_marginal_probabilities /
    // qsim_state_reduced_density_matrix; no reference counterpart).  Qubits follow the gates' and
    // PauliSum's convention, qubit q == index bit q — NOT measure(q)'s big-endian mapping (F2);
    // they are distinct and in any order, and bit j of an output index is qubits[j].
    // std::invalid_argument on a duplicate or too many qubits, std::out_of_range on a bad qubit.
    // 2^k probabilities of the k <= 20 qubits (k = 0: the total probability).
    std::vector<double> marginalProbabilities(const std::vector<int>& qubits) const;
    // rho_A of the k <= 6 qubits, 2^k x 2^k row-major, bitwise equal to its conjugate transpose.
    std::vector<std::complex<double>> reducedDensityMatrix(const std::vector<int>& qubits) const;
    double subsystemPurity(const std::vector<int>& qubits) const;  // Tr rho_A^2
    // Von Neumann entropy of rho_A in bits, -sum l log2 l over its eigenvalues (those below 1e-300
    // contribute 0; a cyclic Jacobi sweep on the host); renyi2: -log2 Tr rho_A^2 instead.
    double entanglementEntropy(const std::vector<int>& qubits, bool renyi2 = false) const;

    // Reference semantics (src/StateVector.cu:260-314): measures index bit n-1-qubit
    // (big-endian), collapses and renormalizes.  std::invalid_argument on a bad
    // qubit, std::runtime_error when the drawn outcome has probability < 1e-15.
    int measure(int qubit);
    // Consistent with the gate convention: measures index bit `bit` (== gate qubit `bit`).
    int measureBit(int bit);
    std::vector<int> sample(int n_shots);  // std::invalid_argument if n_shots <= 0

    // Reproducible measurement/sampling (the reference seeds from std::random_device).
    void setSeed(unsigned int seed);

    qsim_state* handle() const { return h_; }

private:
    int num_qubits_;
    size_t size_;
    qsim_state* h_;
    bool seeded_ = false;
    std::mt19937 rng_;

    // Uniforms on [0,1) from uniform_real_distribution<double> over mt19937, seeded by
    // std::random_device per call (reference) or from setSeed's persistent engine.
    std::vector<double> uniforms(int count);
    void release();
};

// Host helpers behind entanglementEntropy (csrc/host/Marginal.cpp): the ascending eigenvalues of a
// Hermitian dim x dim matrix (row-major) by cyclic Jacobi sweeps, and the entropy in bits of a
// density matrix as defined above.  std::invalid_argument when the size is not dim x dim.
std::vector<double> hermitianEigenvalues(std::vector<std::complex<double>> matrix, int dim);
double hermitianEntropy(const std::vector<std::complex<double>>& rho, int dim, bool renyi2 = false);

}  // namespace qsim
