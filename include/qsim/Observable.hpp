// Observable.hpp — Pauli-sum observables H = sum_t c_t P_t (no reference counterpart: the
// reference has no observable API; a caller reads the amplitudes back and does the sum on the host).
//
// Their expectation values are computed on the device where the state lies
// (qsim_state_expectation / qsim_batch_expectation, include/qsim_hip.h): StateVector::expectation,
// Simulator::expectation, NoisySimulator::expectation, BatchedSimulator::getExpectations; on a
// sharded state DistributedSimulator::expectation (qsim_dist_expectation); on a density matrix
// DensityMatrix::expectation and DensityMatrixSimulator::expectation, Re Tr(rho H)
// (qsim_dm_expectation).
#pragma once

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace qsim {

class PauliSum {
public:
    // One term: bit q of x_mask set where the factor on qubit q is X or Y, of z_mask where it is
    // Z or Y (the layout of qsim_pauli_term).
    struct Term {
        uint64_t x_mask, z_mask;
        double coeff;
    };

    explicit PauliSum(int num_qubits);  // std::invalid_argument outside [1, 30]

    // coeff * the product of the factors (qubit, 'X' | 'Y' | 'Z'); no factors: coeff * identity.
    // std::out_of_range on a bad qubit, std::invalid_argument on a repeated qubit or an unknown
    // letter (the exception types of Circuit).
    PauliSum& add(double coeff, const std::vector<std::pair<int, char>>& factors);

    int getNumQubits() const { return num_qubits_; }
    size_t size() const { return terms_.size(); }
    const std::vector<Term>& terms() const { return terms_; }

private:
    int num_qubits_;
    std::vector<Term> terms_;
};

}  // namespace qsim
