// DensityMatrix.hpp — mixed-state simulation (reference include/DensityMatrix.cuh:63-224).
//
// Host-only header over the qsim_dm_* C ABI (include/qsim_hip.h): rho of n qubits lives in a
// 2n-index-bit engine state (rho[i][j] at i * 2^n + j, the reference's row-major layout), so gates
// and channels run through the same fused HIP passes as a state vector.  n in [1, 15]
// (std::invalid_argument otherwise; the reference allows 1-14).
#pragma once

#include <complex>
#include <random>
#include <vector>

#include "Circuit.hpp"
#include "NoiseModel.hpp"
#include "StateVector.hpp"

namespace qsim {

class DensityMatrix {
public:
    explicit DensityMatrix(int n_qubits);
    DensityMatrix(int n_qubits, const std::vector<std::complex<double>>& pure_state);
    DensityMatrix(DensityMatrix&&) noexcept = default;
    DensityMatrix& operator=(DensityMatrix&&) noexcept = default;

    void reset();
    void initFromPureState(const std::vector<std::complex<double>>& state);
    void initMaximallyMixed();

    int getNumQubits() const { return n_qubits_; }
    size_t getDimension() const { return size_t(1) << n_qubits_; }
    size_t getNumElements() const { return getDimension() * getDimension(); }
    size_t getMemoryBytes() const { return getNumElements() * 16; }

    std::vector<double> getProbabilities() const;
    std::vector<std::complex<double>> getMatrix() const { return rho_.toHost(); }
    double trace() const;
    double purity() const { return rho_.getTotalProbability(); }  // sum |rho_ij|^2
    bool isValid(double tolerance = 1e-10) const;
    // Re Tr(rho H) of a Pauli sum over the n qubits (Observable.hpp), reduced on the device where
    // rho lies: no readback and no layout restore (qsim_dm_expectation).  std::invalid_argument
    // when the observable's qubit count differs.  No reference counterpart.
    double expectation(const PauliSum& observable) const;

    // Readout of a subset of qubits and the fidelity with a pure state, reduced on the device where
    // rho lies (qsim_dm_marginal_probabilities / qsim_dm_reduced_density_matrix / qsim_dm_fidelity;
    // no reference counterpart): no readback of the 4^n elements, no layout restore, linear in
    // whatever the buffer holds (nothing is mirrored or symmetrised), bitwise reproducible.  Qubit
    // q is index bit q; the k qubits are distinct and in any order, and bit j of an output index is
    // qubits[j].  std::invalid_argument on a duplicate or too many qubits, std::out_of_range on a
    // bad qubit (StateVector's exceptions).
    // out[m] = sum_b Re rho[(m, b)][(m, b)]: 2^k doubles, k <= n (k = 0: the trace).
    std::vector<double> marginalProbabilities(const std::vector<int>& qubits) const;
    // rho_A[a][a'] = sum_b rho[(a, b)][(a', b)] of the k <= 6 qubits, 2^k x 2^k row-major.
    std::vector<std::complex<double>> reducedDensityMatrix(const std::vector<int>& qubits) const;
    double subsystemPurity(const std::vector<int>& qubits) const;  // sum |rho_A[a][a']|^2
    // Von Neumann entropy in bits of (rho_A + rho_A^dagger) / 2 by hermitianEntropy (StateVector.hpp);
    // renyi2: -log2 subsystemPurity.  For a mixed rho this is not an entanglement measure; with all
    // n <= 6 qubits it is the entropy of the state itself.
    double subsystemEntropy(const std::vector<int>& qubits, bool renyi2 = false) const;
    // Re sum_ij conj(psi_i) rho[i][j] psi_j in one streaming read of rho; psi (2^n amplitudes) is
    // used as given, not normalised.  std::invalid_argument when its size differs.
    double fidelity(const std::vector<std::complex<double>>& psi) const;

    Amplitude* getDevicePtr() { return rho_.devicePtr(); }
    StateVector& state() { return rho_; }
    const StateVector& state() const { return rho_; }

private:
    int n_qubits_;
    StateVector rho_;
};

class DensityMatrixSimulator {
public:
    explicit DensityMatrixSimulator(int n_qubits, const NoiseModel& noise = NoiseModel());

    void reset() { rho_.reset(); }
    void run(const Circuit& circuit);    // std::runtime_error for CRY/CRZ/Toffoli
    void applyGate(const GateOp& gate);  // unitary only, no noise (src/DensityMatrix.cu:214-267)

    std::vector<double> getProbabilities() const { return rho_.getProbabilities(); }
    std::vector<std::complex<double>> getDensityMatrix() const { return rho_.getMatrix(); }
    double expectation(const PauliSum& observable) const { return rho_.expectation(observable); }
    // DensityMatrix's readout of a subset of qubits and its fidelity, on the device.
    std::vector<double> marginalProbabilities(const std::vector<int>& q) const { return rho_.marginalProbabilities(q); }
    std::vector<std::complex<double>> reducedDensityMatrix(const std::vector<int>& q) const { return rho_.reducedDensityMatrix(q); }
    double subsystemPurity(const std::vector<int>& q) const { return rho_.subsystemPurity(q); }
    double subsystemEntropy(const std::vector<int>& q, bool renyi2 = false) const { return rho_.subsystemEntropy(q, renyi2); }
    double fidelity(const std::vector<std::complex<double>>& psi) const { return rho_.fidelity(psi); }
    double getPurity() const { return rho_.purity(); }
    double getTrace() const { return rho_.trace(); }
    int measureQubit(int qubit);  // index bit `qubit` (src/DensityMatrix.cu:374-406)
    int getNumQubits() const { return rho_.getNumQubits(); }

    void setSeed(unsigned int seed) { rng_.seed(seed); }
    DensityMatrix& density() { return rho_; }
    // Reference results: Y as src/DensityMatrix.cu:507-546 computes it (-Y rho Y^dag); the
    // default is the physical Y rho Y^dag.  (Amplitude damping has no switch: the reference's
    // kernel reads rho11 while another thread rescales it, :1023-1036, so its result is not
    // deterministic; this engine uses the pre-channel rho11, the race-free reading.)
    void setReferenceCompatible(bool on = true) { reference_y_ = on; }

private:
    DensityMatrix rho_;
    NoiseModel noise_model_;
    std::mt19937 rng_;
    bool reference_y_ = false;
};

}  // namespace qsim
