// test_batch_gradient.cpp — BatchedSimulator::gradientSweep of the C++17 layer: the same doubles,
// bitwise, as the C ABI call it wraps (qsim_batch_gradient_sweep), a closed form, the state it leaves,
// and the exception types of runSweep.
#include <qsim/Circuit.hpp>
#include <qsim/NoiseModel.hpp>
#include <qsim/Observable.hpp>
#include <qsim_hip.h>

#include <cmath>
#include <cstring>
#include <random>
#include <stdexcept>
#include <vector>

#include "harness.hpp"

// The test circuit with the angle set `a` (7 parameterised gates; both control orders).
static qsim::Circuit ansatz(int n, const std::vector<double>& a) {
    qsim::Circuit c(n);
    for (int q = 0; q < n; ++q) c.h(q);
    c.rx(0, a[0]).ry(n - 1, a[1]).rz(4, a[2]);
    for (int q = 0; q + 1 < n; ++q) c.cnot(q, q + 1);
    c.cry(1, n - 2, a[3]).crz(n - 1, 2, a[4]).t(3).toffoli(0, 5, 7);
    c.ry(6, a[5]).rz(0, a[6]).swap(2, n - 1);
    return c;
}

static qsim::PauliSum observable(int n) {
    qsim::PauliSum h(n);
    h.add(0.7, {{0, 'Z'}, {9, 'Z'}}).add(-0.4, {{1, 'X'}, {5, 'Y'}}).add(0.3, {{8, 'Y'}}).add(0.2, {{2, 'X'}, {3, 'Z'}});
    // (the four terms above alone have zero energy and gradient on this ansatz, by symmetry)
    h.add(0.5, {{6, 'Z'}}).add(0.35, {{0, 'X'}}).add(0.25, {{4, 'Z'}, {5, 'Z'}}).add(0.45, {{2, 'X'}});
    return h;
}

static bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0);
}

TEST(BatchGradient, SameDoublesAsTheCAbi) {
    const int n = 10, B = 3, P = 7;
    std::mt19937 rng(11);
    std::uniform_real_distribution<double> dist(-3.0, 3.0);
    std::vector<double> angles((size_t)B * P);
    for (double& v : angles) v = dist(rng);
    const qsim::Circuit c = ansatz(n, std::vector<double>(P, 0.123));  // (the stored angles are ignored)
    const qsim::PauliSum h = observable(n);
    qsim::BatchedSimulator batch(n, B);
    batch.setNoiseSemantics(qsim::BatchedNoise::Physical);
    const qsim::BatchedSimulator::SweepGradient got = batch.gradientSweep(c, angles, h);
    ASSERT_TRUE(got.values.size() == (size_t)B && got.gradients.size() == (size_t)B * P);
    // the values are what getExpectations returns for the state the call leaves
    EXPECT_TRUE(same_bits(got.values, batch.getExpectations(h)));

    std::vector<qsim_gate> gates;
    for (const qsim::GateOp& g : c.getGates()) {
        qsim_gate r{};
        r.type = static_cast<int>(g.type);
        r.nqubits = (int)g.qubits.size();
        for (size_t i = 0; i < g.qubits.size() && i < 3; ++i) r.qubits[i] = g.qubits[i];
        r.parameter = g.parameter;
        gates.push_back(r);
    }
    std::vector<qsim_pauli_term> terms;
    for (const qsim::PauliSum::Term& t : h.terms()) terms.push_back(qsim_pauli_term{t.x_mask, t.z_mask, t.coeff});
    qsim::BatchedSimulator raw(n, B);
    std::vector<double> values((size_t)B, -1.0), grads((size_t)B * P, -1.0);
    ASSERT_TRUE(qsim_batch_gradient_sweep(raw.handle(), gates.data(), gates.size(), angles.data(), P, terms.data(),
                                          terms.size(), 0, values.data(), grads.data()) == QSIM_OK);
    EXPECT_TRUE(same_bits(got.values, values));
    EXPECT_TRUE(same_bits(got.gradients, grads));
    bool any = false;
    for (double g : grads) any = any || std::fabs(g) > 1e-3;
    EXPECT_TRUE(any);
    // both objects hold the same members
    for (int t = 0; t < B; ++t) EXPECT_TRUE(same_bits(batch.getProbabilities(t), raw.getProbabilities(t)));
    // released and allocated again: the same doubles
    batch.releaseGradientBuffers();
    batch.reset();
    const qsim::BatchedSimulator::SweepGradient again = batch.gradientSweep(c, angles, h);
    EXPECT_TRUE(same_bits(again.values, values));
    EXPECT_TRUE(same_bits(again.gradients, grads));
}

TEST(BatchGradient, ClosedForm) {
    // RY(theta_t) on every qubit, then a CZ ladder (diagonal: commutes with every Z); H = sum_q Z_q
    const int n = 6, B = 4;
    qsim::Circuit c(n);
    qsim::PauliSum h(n);
    for (int q = 0; q < n; ++q) {
        c.ry(q, 0.0);
        h.add(1.0, {{q, 'Z'}});
    }
    for (int q = 0; q + 1 < n; ++q) c.cz(q, q + 1);
    std::vector<double> angles((size_t)B * n);
    for (int t = 0; t < B; ++t)
        for (int q = 0; q < n; ++q) angles[(size_t)t * n + q] = 0.2 + 0.25 * q - 0.4 * t;
    qsim::BatchedSimulator batch(n, B);
    batch.setNoiseSemantics(qsim::BatchedNoise::Physical);
    const qsim::BatchedSimulator::SweepGradient g = batch.gradientSweep(c, angles, h);
    for (int t = 0; t < B; ++t) {
        double e = 0.0;
        for (int q = 0; q < n; ++q) {
            e += std::cos(angles[(size_t)t * n + q]);
            EXPECT_NEAR(g.gradients[(size_t)t * n + q], -std::sin(angles[(size_t)t * n + q]), 1e-12 * n);
        }
        EXPECT_NEAR(g.values[t], e, 1e-12 * n);
    }
}

TEST(BatchGradient, Exceptions) {
    const int n = 10, B = 3, P = 7;
    const qsim::Circuit c = ansatz(n, std::vector<double>(P, 0.5));
    const qsim::PauliSum h = observable(n);
    const std::vector<double> good((size_t)B * P, 0.1);
    qsim::BatchedSimulator batch(n, B);
    // the default noise semantics is the reference's
    EXPECT_THROW(batch.gradientSweep(c, good, h), std::invalid_argument);
    batch.setNoiseSemantics(qsim::BatchedNoise::Physical);
    EXPECT_THROW(batch.gradientSweep(c, std::vector<double>((size_t)B * P - 1, 0.1), h), std::invalid_argument);
    EXPECT_THROW(batch.gradientSweep(c, std::vector<double>((size_t)P, 0.1), h), std::invalid_argument);
    EXPECT_THROW(batch.gradientSweep(qsim::Circuit(n + 1), {}, h), std::invalid_argument);
    EXPECT_THROW(batch.gradientSweep(c, good, qsim::PauliSum(n + 1)), std::invalid_argument);
    qsim::NoiseModel nm;
    nm.addDepolarizing({0}, 0.1);
    batch.setNoiseModel(nm);
    EXPECT_THROW(batch.gradientSweep(c, good, h), std::invalid_argument);
    batch.setNoiseModel(qsim::NoiseModel());
    batch.setGateSet(qsim::BatchedGateSet::Reference);
    EXPECT_THROW(batch.gradientSweep(c, good, h), std::invalid_argument);
    batch.setGateSet(qsim::BatchedGateSet::Full);
    // nothing ran: every trajectory is still |0...0>
    const std::vector<double> p = batch.getProbabilities(1);
    EXPECT_NEAR(p[0], 1.0, 0.0);
    EXPECT_NO_THROW(batch.releaseGradientBuffers());  // nothing to release yet
    const qsim::BatchedSimulator::SweepGradient g = batch.gradientSweep(c, good, h);  // and the object still works
    EXPECT_TRUE(g.values.size() == (size_t)B && g.gradients.size() == (size_t)B * P);
}

TH_MAIN
