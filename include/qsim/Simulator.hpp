// Simulator.hpp — circuit execution on one MI355X (reference include/Simulator.hpp:53-85).
//
// Drop-in for the reference `Simulator`: same constructor, run/applyGate, readout, sampling and
// measurement signatures and exception types.  run() is asynchronous like the reference
// (src/Simulator.cu:95-97); every readout synchronizes.  By default run() hands the whole circuit
// to the engine's fused-pass planner (RunMode::Fused); RunMode::PerGate reproduces the
// reference's one-launch-per-gate execution.
//
// CPUSimulator (reference include/Simulator.hpp:91-112, src/Simulator.cu:195-345) is this
// library's own host implementation (csrc/host/CPUSimulator.cpp: gate table + thread pool over
// the amplitude pairs), kept for code that compares against the CPU (benchmark_scaling.cu:85).
// It is not the parity oracle (oracle/ is test infrastructure and is never linked here).
#pragma once

#include <complex>
#include <cstdint>
#include <memory>
#include <random>
#include <vector>

#include "Circuit.hpp"
#include "StateVector.hpp"

namespace qsim {

enum class RunMode { PerGate, Fused };

// Result of Simulator::gradient: the expectation value and dE/dtheta per gate of the circuit.
struct Gradient {
    double value;
    std::vector<double> gradient;
};

class Simulator {
public:
    explicit Simulator(int num_qubits);

    void reset();
    void run(const Circuit& circuit);  // std::invalid_argument on qubit-count mismatch
    // run() of each circuit in turn as ONE engine run (no reference counterpart): the planner
    // sees their gates together, so a fused pass may hold the end of one and the start of the
    // next (consecutive W-HC circuits at 30 qubits: 2.5-2.75 passes each instead of 4).
    void runSequence(const std::vector<Circuit>& circuits);
    void applyGate(const GateOp& gate);

    std::vector<std::complex<double>> getStateVector() const;
    std::vector<double> getProbabilities() const;

    std::vector<int> sample(int n_shots);  // without collapse
    int measureQubit(int qubit);           // reference semantics: StateVector::measure (F2)
    // <psi|H|psi> of a Pauli sum on the device (no reference counterpart; StateVector::expectation).
    double expectation(const PauliSum& observable) const;
    // Runs `circuit` on the state as it is (as run() would, in `mode`), then returns <psi|H|psi>
    // and its derivative with respect to the angle of every gate (one entry per gate, 0 for a gate
    // without a parameter) by the adjoint method: one backward sweep on the device, one pass over
    // two work states per angle, instead of two circuit runs per angle (qsim_state_gradient).
    // The state is left as run() leaves it.  std::invalid_argument on a qubit-count mismatch; no
    // reference counterpart.
    Gradient gradient(const Circuit& circuit, const PauliSum& observable, RunMode mode = RunMode::Fused);
    void releaseGradientBuffers();  // free the two work states gradient() keeps between calls
    // Pauli-string rotations (no reference counterpart): StateVector::applyPauliRotation(s).
    void applyPauliRotation(const std::vector<std::pair<int, char>>& factors, double theta);
    void applyPauliRotations(const PauliSum& seq);
    // The Trotter product for exp(-i H time) on the state as it is: nothing but
    // applyPauliRotations(trotter_sequence(H, time, steps, order)) (Observable.hpp defines both
    // orders).  std::invalid_argument when steps < 1, order is not 1 or 2 or the qubit counts differ.
    void evolve(const PauliSum& H, double time, int steps = 1, int order = 1);
    // Applies the rotation sequence `seq` (a PauliSum read in add() order) to the state as it is,
    // then returns <psi|H|psi> and its derivative with respect to the angle of every rotation (one
    // entry per term of seq) by the adjoint method: one backward sweep on the device, one fused
    // pass over two work states per rotation (qsim_state_pauli_gradient).  The state is left as
    // applyPauliRotations(seq) leaves it.  The angles are independent parameters: a parameter
    // shared between rotations (a QAOA gamma) is the caller's chain rule over the gradient.
    Gradient pauliGradient(const PauliSum& seq, const PauliSum& observable);
    // Readout of a subset of qubits on the device (no reference counterpart): StateVector's methods.
    std::vector<double> marginalProbabilities(const std::vector<int>& qubits) const;
    std::vector<std::complex<double>> reducedDensityMatrix(const std::vector<int>& qubits) const;
    double subsystemPurity(const std::vector<int>& qubits) const;
    double entanglementEntropy(const std::vector<int>& qubits, bool renyi2 = false) const;

    int getNumQubits() const { return state_.getNumQubits(); }
    size_t getStateSize() const { return state_.getSize(); }

    void setRunMode(RunMode m) { mode_ = m; }
    RunMode getRunMode() const { return mode_; }
    void setSeed(unsigned int seed) { state_.setSeed(seed); }
    void synchronize() const;
    StateVector& state() { return state_; }
    const StateVector& state() const { return state_; }

private:
    StateVector state_;
    RunMode mode_ = RunMode::Fused;
};

// Which gates CPUSimulator::applyGate acts on.  Reference: exactly the reference CPU path —
// every 1-qubit gate, CNOT, CZ and SWAP; CRY, CRZ and Toffoli are silent no-ops
// (src/Simulator.cu:214-220, 313-314).  Full: CRY / CRZ / Toffoli as the GPU kernels
// define them (src/Gates.cu:322-410), so CPU and GPU agree on every circuit.
enum class CpuGateSet { Reference, Full };

class CPUSimulator {
public:
    explicit CPUSimulator(int num_qubits, CpuGateSet gates = CpuGateSet::Reference);

    void reset();
    void run(const Circuit& circuit);  // std::invalid_argument on qubit-count mismatch
    void applyGate(const GateOp& gate);

    std::vector<std::complex<double>> getStateVector() const { return state_; }
    std::vector<double> getProbabilities() const;
    std::vector<int> sample(int n_shots);

    int getNumQubits() const { return num_qubits_; }
    size_t getStateSize() const { return state_.size(); }

    // Worker threads for the pair loops (a persistent pool; default min(hardware threads, 16);
    // states below 2^17 amplitudes always run on the calling thread).  1 = the reference's single
    // core.
    void setThreads(int threads);
    int getThreads() const { return threads_; }
    void setSeed(unsigned int seed) { rng_.seed(seed); }

private:
    int num_qubits_;
    CpuGateSet gate_set_;
    int threads_;
    std::vector<std::complex<double>> state_;
    std::mt19937 rng_;
    struct Pool;
    std::shared_ptr<Pool> pool_;
};

}  // namespace qsim
