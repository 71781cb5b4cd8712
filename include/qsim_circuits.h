/*
 * qsim_circuits.h — C ABI of the C++ circuit factories in libqsim.so.
 *
 * Lets non-C++ hosts (the Python ctypes mirror, bench.py) obtain gate lists that are identical to
 * the reference's libstdc++ factories (std::mt19937 + uniform_*_distribution draw order of
 * src/Circuit.cpp:234-282), instead of re-implementing the distributions.
 */
#ifndef QSIM_CIRCUITS_H
#define QSIM_CIRCUITS_H

#include <stddef.h>

#include "qsim_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    QSIM_CIRCUIT_BELL = 0,      /* createBellCircuit()                    Circuit.cpp:234-238 */
    QSIM_CIRCUIT_GHZ = 1,       /* createGHZCircuit(n)                    Circuit.cpp:240-250 */
    QSIM_CIRCUIT_RANDOM = 2,    /* createRandomCircuit(n, depth, seed)    Circuit.cpp:252-282 */
    QSIM_CIRCUIT_RANDOM_HC = 3, /* W-HC: random {H, CNOT}, same draw order */
    QSIM_CIRCUIT_SCALING = 4    /* W-REF: benchmarks/benchmark_scaling.cu:69-76 */
};

/* Writes up to `cap` gates to `out` and the full gate count to *count (call with cap = 0 to size).
 * Returns QSIM_OK or a QSIM_ERR_* code (message in qsim_circuits_last_error()). */
int qsim_circuit_make(int kind, int n_qubits, int depth, unsigned int seed, qsim_gate* out,
                      size_t cap, size_t* count);
/* Circuit::getDepth() of a gate list (Circuit.cpp:183-201). */
int qsim_circuit_depth(int n_qubits, const qsim_gate* gates, size_t count, size_t* depth);
const char* qsim_circuits_last_error(void);
/* One qsim::PauliSum::add (include/qsim/Observable.hpp) through the C ABI: the term coeff * the
 * product of the `count` factors (qubits[i], letters[i] in "XYZ") on n_qubits qubits, with that
 * method's argument checks (QSIM_ERR_OUT_OF_RANGE / QSIM_ERR_INVALID_ARGUMENT).  Part of the
 * public interface of libqsim.so like the circuit factories above: it lets a non-C++ host build
 * qsim_pauli_term masks with the C++ layer's checks (the Python tests reach PauliSum through it);
 * it sets no message in qsim_circuits_last_error(). */
int qsim_pauli_term_make(int n_qubits, const int32_t* qubits, const char* letters, size_t count,
                         double coeff, qsim_pauli_term* out);
/* qsim::hermitianEntropy (include/qsim/StateVector.hpp) through the C ABI: the entropy in bits of
 * the dim x dim density matrix rho (row-major, interleaved re/im, 1 <= dim <= 64), von Neumann from
 * the host's cyclic Jacobi eigenvalues, or -log2 Tr rho^2 with renyi2 != 0.  Lets a non-C++ host
 * check the routine behind StateVector::entanglementEntropy; null pointers or a bad dim ->
 * QSIM_ERR_INVALID_ARGUMENT. */
int qsim_hermitian_entropy(const double* rho, int dim, int renyi2, double* out);

#ifdef __cplusplus
}
#endif
#endif /* QSIM_CIRCUITS_H */
