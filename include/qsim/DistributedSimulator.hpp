// DistributedSimulator.hpp — the state sharded over the GPUs of one node, one process per GPU
// (qsim_dist_* of qsim_hip.h; no reference counterpart: the reference is single-GPU).
//
// `Simulator`'s run / readout / sampling / measurement signatures and exception types on a
// sharded state.  Every method that touches the state is collective: every rank calls it with
// the same arguments.  Gathered readouts (getStateVector, getProbabilities) return the result on
// rank 0 and an empty vector elsewhere; sample() and measureQubit() return the same values on
// every rank (rank 0 draws the uniforms and broadcasts them).  sample() gathers nothing, but may
// move qubits between rank and local positions (the amplitudes are unchanged).
//
//   rank 0:  auto id = DistributedSimulator::uniqueId();   // then hand `id` to the other ranks
//   rank r:  DistributedSimulator sim(30, r, 8, id, /*device=*/r);
//
// makeVirtual(n, world) keeps all `world` shards in this process on one GPU (exchanges by device
// copies): the same planner and kernels, for running the sharded path on a single GPU.
#pragma once

#include <array>
#include <complex>
#include <random>
#include <vector>

#include "Circuit.hpp"
#include "Observable.hpp"
#include "Simulator.hpp"

struct qsim_dist;

namespace qsim {

class DistributedSimulator {
public:
    using UniqueId = std::array<unsigned char, 128>;

    DistributedSimulator(int num_qubits, int rank, int world, const UniqueId& unique_id, int device);
    ~DistributedSimulator();
    DistributedSimulator(DistributedSimulator&& o) noexcept;
    DistributedSimulator& operator=(DistributedSimulator&& o) noexcept;
    DistributedSimulator(const DistributedSimulator&) = delete;
    DistributedSimulator& operator=(const DistributedSimulator&) = delete;

    static UniqueId uniqueId();  // on rank 0
    static DistributedSimulator makeVirtual(int num_qubits, int world, int device = 0);

    void reset();
    void run(const Circuit& circuit);  // std::invalid_argument on qubit-count mismatch
    void runSequence(const std::vector<Circuit>& circuits);

    std::vector<std::complex<double>> getStateVector() const;  // rank 0; empty elsewhere
    std::vector<double> getProbabilities() const;              // rank 0; empty elsewhere

    // <psi|H|psi> of a Pauli sum (Observable.hpp) on the sharded state, the same value on every
    // rank: every shard is read where it lies, nothing is gathered and no qubit moves
    // (qsim_dist_expectation).  std::invalid_argument on a qubit-count mismatch.
    double expectation(const PauliSum& observable) const;

    // StateVector's readout of a subset of qubits on the sharded state, the same values on every
    // rank (qsim_dist_marginal_probabilities / qsim_dist_reduced_density_matrix): every shard is
    // read where it lies, nothing is gathered and no qubit moves; a matrix over qubits that sit
    // on rank positions pairs ranks and moves at most a shard each way per pair step.
    // StateVector's conventions (qubit q == index bit q, bit j of an output index is qubits[j]),
    // caps (20 / 6 qubits) and exceptions: std::invalid_argument on a duplicate or too many
    // qubits, std::out_of_range on a bad qubit.  Purity and entropy as StateVector's (the entropy
    // through hermitianEntropy's Jacobi sweep).
    std::vector<double> marginalProbabilities(const std::vector<int>& qubits) const;
    std::vector<std::complex<double>> reducedDensityMatrix(const std::vector<int>& qubits) const;
    double subsystemPurity(const std::vector<int>& qubits) const;
    double entanglementEntropy(const std::vector<int>& qubits, bool renyi2 = false) const;

    // Simulator::gradient on the sharded state (collective, qsim_dist_gradient): runs `circuit` as
    // run() would in `mode`, then <psi|H|psi> and its derivative with respect to the angle of every
    // gate by one backward sweep over two sharded work states; a rotation whose target sits on a
    // rank position pairs each rank with one peer instead of remapping.  The same values on every
    // rank; the state and its qubit map are left as run() leaves them.  std::invalid_argument on a
    // qubit-count mismatch.
    Gradient gradient(const Circuit& circuit, const PauliSum& observable, RunMode mode = RunMode::Fused);
    void releaseGradientBuffers();  // free the two work shards per rank gradient() keeps between calls

    // Simulator's Pauli-string rotations on the sharded state (collective,
    // qsim_dist_apply_pauli_rotations): exp(-i theta/2 P) in add() order where the shards lie, no
    // remap and the qubit map unchanged.  A run of consecutive Z/I-only rotations is one pass per
    // shard, a rotation with X or Y factors on local positions only one pass per shard; one with an
    // X or Y factor on a qubit that sits on a rank position pairs each rank with one peer and moves
    // a whole shard each way.  Exceptions as on Simulator.
    void applyPauliRotation(const std::vector<std::pair<int, char>>& factors, double theta);
    void applyPauliRotations(const PauliSum& seq);
    // applyPauliRotations(trotter_sequence(H, time, steps, order)).
    void evolve(const PauliSum& H, double time, int steps = 1, int order = 1);
    // Simulator::pauliGradient on the sharded state (collective, qsim_dist_pauli_gradient): applies
    // `seq`, then <psi|H|psi> and its derivative with respect to every rotation's angle by one
    // backward sweep over the work shards of gradient().  The same values on every rank; the state
    // is left as applyPauliRotations(seq) leaves it.
    Gradient pauliGradient(const PauliSum& seq, const PauliSum& observable);

    std::vector<int> sample(int n_shots);  // without collapse; the same shots on every rank
    int measureQubit(int qubit);           // reference semantics: index bit n-1-qubit (F2)

    int getNumQubits() const { return num_qubits_; }
    int getWorldSize() const { return world_; }
    int getRank() const { return rank_; }

    void setRunMode(RunMode m) { mode_ = m; }
    RunMode getRunMode() const { return mode_; }
    void setSeed(unsigned int seed);
    void synchronize() const;

private:
    DistributedSimulator() = default;
    std::vector<double> uniforms(int count);
    bool root() const { return virtual_ || rank_ == 0; }

    qsim_dist* h_ = nullptr;
    int num_qubits_ = 0, rank_ = 0, world_ = 1;
    bool virtual_ = false;
    RunMode mode_ = RunMode::Fused;
    bool seeded_ = false;
    std::mt19937 rng_;
};

}  // namespace qsim
