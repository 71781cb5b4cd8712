// test_dist_pauli_rotation.cpp — qsim::DistributedSimulator::applyPauliRotation(s) / evolve /
// pauliGradient (include/qsim/DistributedSimulator.hpp) on 8 virtual ranks at 12 qubits: all four
// calls in turn from |0..0> (qubits 9 .. 11 sit on rank positions), against qsim::Simulator at
// 1e-12, the state after pauliGradient, the exception types.  With QSIM_TEST_DUMP set to a file name
// the case also writes its value, gradient and final amplitudes there as hex floats, for
// tests/test_dist_pauli_rotation_cpp.py to compare with numpy.
#include <qsim/DistributedSimulator.hpp>
#include <qsim/Observable.hpp>
#include <qsim/Simulator.hpp>

#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#include "harness.hpp"

namespace {
constexpr int kN = 12;
const char kLetters[3] = {'X', 'Y', 'Z'};

// Rotation k of the sequence: every third one Z-only, the others X / Y / Z on three qubits.
// tests/test_dist_pauli_rotation_cpp.py restates these formulas.
qsim::PauliSum sequence() {
    qsim::PauliSum seq(kN);
    for (int k = 0; k < kN; ++k) {
        if (k % 3 == 2)
            seq.add(0.1 * (k + 1), {{k, 'Z'}, {(k + 3) % kN, 'Z'}});
        else
            seq.add(-0.15 * (k + 1), {{k, kLetters[k % 2]}, {(k + 5) % kN, 'Y'}, {(k + 7) % kN, 'Z'}});
    }
    return seq;
}

qsim::PauliSum observable(double* sum_abs) {
    qsim::PauliSum h(kN);
    *sum_abs = 0.0;
    for (int q = 0; q < kN; ++q) {
        h.add(0.3 + 0.05 * q, {{q, 'Z'}, {(q + 1) % kN, 'Z'}});
        h.add(-0.2 - 0.01 * q, {{q, 'X'}});
        h.add(0.15, {{q, 'Y'}, {(q + 5) % kN, 'X'}});
        *sum_abs += 0.3 + 0.05 * q + 0.2 + 0.01 * q + 0.15;
    }
    return h;
}

qsim::PauliSum tfim() {
    qsim::PauliSum h(kN);
    for (int q = 0; q + 1 < kN; ++q) h.add(-1.0, {{q, 'Z'}, {q + 1, 'Z'}});
    for (int q = 0; q < kN; ++q) h.add(-0.7, {{q, 'X'}});
    return h;
}

double maxDiff(const std::vector<std::complex<double>>& a, const std::vector<std::complex<double>>& b) {
    double e = 0.0;
    for (size_t i = 0; i < a.size(); ++i)
        e = std::max(e, std::max(std::abs(a[i].real() - b[i].real()), std::abs(a[i].imag() - b[i].imag())));
    return e;
}
}  // namespace

TEST(DistPauliRotation, AllFourCallsMatchSimulator) {
    double sum_abs = 0.0;
    const qsim::PauliSum seq = sequence(), h = observable(&sum_abs), ham = tfim();
    qsim::DistributedSimulator d = qsim::DistributedSimulator::makeVirtual(kN, 8);
    qsim::DistributedSimulator twin = qsim::DistributedSimulator::makeVirtual(kN, 8);
    qsim::Simulator sim(kN);
    d.applyPauliRotation({{0, 'X'}, {11, 'Y'}, {5, 'Z'}}, 0.7);
    twin.applyPauliRotation({{0, 'X'}, {11, 'Y'}, {5, 'Z'}}, 0.7);
    sim.applyPauliRotation({{0, 'X'}, {11, 'Y'}, {5, 'Z'}}, 0.7);
    d.evolve(ham, 0.4, 2, 2);
    twin.evolve(ham, 0.4, 2, 2);
    sim.evolve(ham, 0.4, 2, 2);
    EXPECT_TRUE(maxDiff(d.getStateVector(), sim.getStateVector()) < 1e-12);
    const qsim::Gradient g = d.pauliGradient(seq, h);
    const qsim::Gradient want = sim.pauliGradient(seq, h);
    EXPECT_NEAR(g.value, want.value, 1e-12 * sum_abs);
    EXPECT_TRUE(g.gradient.size() == want.gradient.size() && (int)g.gradient.size() == kN);
    for (size_t k = 0; k < g.gradient.size(); ++k) EXPECT_NEAR(g.gradient[k], want.gradient[k], 1e-12 * sum_abs);
    twin.applyPauliRotations(seq);
    EXPECT_TRUE(d.getStateVector() == twin.getStateVector());  // the state: what applyPauliRotations alone leaves
    EXPECT_NEAR(d.expectation(h), g.value, 0.0);
    d.releaseGradientBuffers();
    d.applyPauliRotations(seq);
    sim.applyPauliRotations(seq);
    const std::vector<std::complex<double>> psi = d.getStateVector();
    EXPECT_TRUE(maxDiff(psi, sim.getStateVector()) < 1e-12);
    if (const char* path = std::getenv("QSIM_TEST_DUMP")) {
        std::FILE* f = std::fopen(path, "w");
        EXPECT_TRUE(f != nullptr);
        if (f) {
            std::fprintf(f, "%a\n", g.value);
            for (double v : g.gradient) std::fprintf(f, "%a\n", v);
            for (const std::complex<double>& a : psi) std::fprintf(f, "%a %a\n", a.real(), a.imag());
            std::fclose(f);
        }
    }
}

TEST(DistPauliRotation, WorldOne) {
    double sum_abs = 0.0;
    const qsim::PauliSum seq = sequence(), h = observable(&sum_abs);
    qsim::DistributedSimulator d = qsim::DistributedSimulator::makeVirtual(kN, 1);
    qsim::Simulator sim(kN);
    const qsim::Gradient g = d.pauliGradient(seq, h), want = sim.pauliGradient(seq, h);
    EXPECT_NEAR(g.value, want.value, 1e-12 * sum_abs);
    for (size_t k = 0; k < g.gradient.size(); ++k) EXPECT_NEAR(g.gradient[k], want.gradient[k], 1e-12 * sum_abs);
    EXPECT_TRUE(d.getStateVector() == sim.getStateVector());  // the same kernels with the same arguments
}

TEST(DistPauliRotation, Exceptions) {
    qsim::DistributedSimulator d = qsim::DistributedSimulator::makeVirtual(kN, 8);
    qsim::PauliSum h(kN), wrong(kN - 1);
    h.add(1.0, {{0, 'Z'}});
    wrong.add(1.0, {{0, 'X'}});
    EXPECT_THROW(d.applyPauliRotation({{kN, 'X'}}, 0.3), std::out_of_range);
    EXPECT_THROW(d.applyPauliRotations(wrong), std::invalid_argument);
    EXPECT_THROW(d.evolve(wrong, 1.0), std::invalid_argument);
    EXPECT_THROW(d.evolve(h, 1.0, 0, 1), std::invalid_argument);
    EXPECT_THROW(d.pauliGradient(wrong, h), std::invalid_argument);
    EXPECT_THROW(d.pauliGradient(h, wrong), std::invalid_argument);
    const qsim::Gradient g = d.pauliGradient(qsim::PauliSum(kN), h);  // no rotation: the value of |0..0>
    EXPECT_NEAR(g.value, 1.0, 1e-15);
    EXPECT_TRUE(g.gradient.empty());
}

TH_MAIN
