// test_pauli_rotation.cpp — the Pauli-rotation API of the C++17 layer: StateVector::applyPauliRotation(s)
// against closed forms and the circuit gates, trotter_sequence term for term, Simulator::evolve
// against an exactly solvable H, Simulator::pauliGradient against closed forms and the exact
// +-pi/2 shift, and the exception types.
#include <qsim/Circuit.hpp>
#include <qsim/Observable.hpp>
#include <qsim/Simulator.hpp>
#include <qsim/StateVector.hpp>

#include <cmath>
#include <complex>
#include <stdexcept>
#include <utility>
#include <vector>

#include "harness.hpp"

using cplx = std::complex<double>;

static double worst(const std::vector<cplx>& a, const std::vector<cplx>& b) {
    double w = a.size() == b.size() ? 0.0 : 1.0;
    for (size_t i = 0; i < a.size() && i < b.size(); ++i)
        w = std::fmax(w, std::fmax(std::fabs(a[i].real() - b[i].real()), std::fabs(a[i].imag() - b[i].imag())));
    return w;
}

TEST(PauliRotation, ClosedForms) {
    const double th = 0.61, c = std::cos(th / 2), s = std::sin(th / 2), tol = 1e-12;
    {
        qsim::Simulator sim(2);
        sim.applyPauliRotation({{0, 'X'}, {1, 'X'}}, th);  // cos |00> - i sin |11>
        EXPECT_NEAR(worst(sim.getStateVector(), {cplx(c, 0), 0, 0, cplx(0, -s)}), 0.0, tol);
    }
    {
        qsim::Simulator sim(2);
        qsim::Circuit plus(2);
        plus.h(0).h(1);
        sim.run(plus);
        sim.state().applyPauliRotation({{0, 'Z'}, {1, 'Z'}}, th);
        const cplx m(c / 2, -s / 2), p(c / 2, s / 2);
        EXPECT_NEAR(worst(sim.getStateVector(), {m, p, p, m}), 0.0, tol);
        sim.applyPauliRotation({}, th);  // the identity string: exp(-i theta/2)
        const cplx ph(c, -s);
        EXPECT_NEAR(worst(sim.getStateVector(), {m * ph, p * ph, p * ph, m * ph}), 0.0, tol);
    }
    // weight-1 rotations are the gates of Circuit, global phase included
    const int n = 5;
    const qsim::Circuit prep = qsim::createRandomCircuit(n, 40, 3);
    for (int q : {0, 4}) {
        for (char letter : {'X', 'Y', 'Z'}) {
            qsim::Simulator a(n), b(n);
            a.run(prep);
            b.run(prep);
            a.applyPauliRotation({{q, letter}}, th);
            qsim::Circuit g(n);
            if (letter == 'X') g.rx(q, th);
            if (letter == 'Y') g.ry(q, th);
            if (letter == 'Z') g.rz(q, th);
            b.setRunMode(qsim::RunMode::PerGate);
            b.run(g);
            EXPECT_NEAR(worst(a.getStateVector(), b.getStateVector()), 0.0, tol);
        }
    }
}

TEST(PauliRotation, TrotterSequence) {
    qsim::PauliSum h(3);
    h.add(-1.0, {{0, 'Z'}, {1, 'Z'}}).add(-0.5, {{1, 'Z'}, {2, 'Z'}}).add(0.7, {{0, 'X'}});
    const double time = 0.9;
    const qsim::PauliSum o1 = qsim::trotter_sequence(h, time, 3, 1);
    ASSERT_TRUE(o1.size() == 9);
    for (size_t k = 0; k < 9; ++k) {
        EXPECT_TRUE(o1.terms()[k].x_mask == h.terms()[k % 3].x_mask && o1.terms()[k].z_mask == h.terms()[k % 3].z_mask);
        EXPECT_NEAR(o1.terms()[k].coeff, 2.0 * h.terms()[k % 3].coeff * time / 3, 1e-15);
    }
    // order 2, two steps: 0/2 1/2 2 1/2 [0] 1/2 2 1/2 0/2, the term-0 halves between the steps merged
    const qsim::PauliSum o2 = qsim::trotter_sequence(h, time, 2, 2);
    const int want_term[9] = {0, 1, 2, 1, 0, 1, 2, 1, 0};
    const double want_scale[9] = {0.5, 0.5, 1.0, 0.5, 1.0, 0.5, 1.0, 0.5, 0.5};
    ASSERT_TRUE(o2.size() == 9);
    for (size_t k = 0; k < 9; ++k) {
        const qsim::PauliSum::Term& t = h.terms()[want_term[k]];
        EXPECT_TRUE(o2.terms()[k].x_mask == t.x_mask && o2.terms()[k].z_mask == t.z_mask);
        EXPECT_NEAR(o2.terms()[k].coeff, want_scale[k] * 2.0 * t.coeff * time / 2, 1e-15);
    }
    EXPECT_EQ(qsim::trotter_sequence(h, time).size(), (size_t)3);
    EXPECT_EQ(qsim::trotter_sequence(qsim::PauliSum(3), time, 2, 2).size(), (size_t)0);
    EXPECT_THROW(qsim::trotter_sequence(h, time, 0, 1), std::invalid_argument);
    EXPECT_THROW(qsim::trotter_sequence(h, time, 1, 3), std::invalid_argument);
    EXPECT_THROW(qsim::trotter_sequence(h, time, 1, 0), std::invalid_argument);
}

TEST(PauliRotation, Evolve) {
    // H = w X on one qubit: exp(-i H t)|0> = cos(wt)|0> - i sin(wt)|1>, exact at every order
    const double w = 0.8, t = 1.7, tol = 1e-12;
    qsim::PauliSum hx(1);
    hx.add(w, {{0, 'X'}});
    for (int order : {1, 2}) {
        qsim::Simulator sim(1);
        sim.evolve(hx, t, 4, order);
        EXPECT_NEAR(worst(sim.getStateVector(), {cplx(std::cos(w * t), 0), cplx(0, -std::sin(w * t))}), 0.0, tol);
    }
    // a commuting (Z-only) H on |+...+>: amplitude i gets exp(-i t E_i), E_i the diagonal of H
    const int n = 6;
    qsim::PauliSum hz(n);
    hz.add(0.9, {{0, 'Z'}, {1, 'Z'}}).add(-0.4, {{2, 'Z'}}).add(0.3, {{1, 'Z'}, {4, 'Z'}, {5, 'Z'}}).add(0.2, {});
    qsim::Circuit plus(n);
    for (int q = 0; q < n; ++q) plus.h(q);
    std::vector<cplx> want((size_t)1 << n);
    for (size_t i = 0; i < want.size(); ++i) {
        double e = 0.0;
        for (const qsim::PauliSum::Term& term : hz.terms())
            e += (__builtin_popcountll(i & term.z_mask) & 1 ? -1.0 : 1.0) * term.coeff;
        want[i] = std::polar(1.0 / 8.0, -t * e);
    }
    for (int order : {1, 2}) {
        qsim::Simulator sim(n);
        sim.run(plus);
        sim.evolve(hz, t, 3, order);
        EXPECT_NEAR(worst(sim.getStateVector(), want), 0.0, tol);
    }
    qsim::Simulator sim(n);
    EXPECT_THROW(sim.evolve(hz, t, 0), std::invalid_argument);
    EXPECT_THROW(sim.evolve(hz, t, 1, 4), std::invalid_argument);
    EXPECT_THROW(sim.evolve(hx, t), std::invalid_argument);  // qubit-count mismatch
}

TEST(PauliRotation, GradientClosedFormAndShift) {
    const double th = 0.73, tol = 1e-12;
    qsim::PauliSum z(1);
    z.add(1.0, {{0, 'Z'}});
    {
        qsim::Simulator s(1);
        qsim::PauliSum seq(1);
        seq.add(0.0, {{0, 'Z'}}).add(th, {{0, 'X'}});  // E = cos theta
        const qsim::Gradient g = s.pauliGradient(seq, z);
        ASSERT_TRUE(g.gradient.size() == 2);
        EXPECT_NEAR(g.value, std::cos(th), tol);
        EXPECT_NEAR(g.gradient[1], -std::sin(th), tol);
        EXPECT_NEAR(s.expectation(z), g.value, 0.0);  // the state holds the rotated state
    }
    const int n = 8;
    qsim::PauliSum h(n);
    double abs_sum = 0.0;
    for (int q = 0; q + 1 < n; ++q) {
        h.add(-1.0, {{q, 'Z'}, {q + 1, 'Z'}});
        abs_sum += 1.0;
    }
    h.add(0.25, {{0, 'Y'}, {3, 'X'}, {5, 'Y'}}).add(-0.5, {{7, 'X'}});
    abs_sum += 0.75;
    std::vector<double> angles(7);
    for (size_t i = 0; i < angles.size(); ++i) angles[i] = 0.2 + 0.41 * (double)i;
    auto sequence = [&](const std::vector<double>& a) {
        qsim::PauliSum seq(n);
        seq.add(a[0], {{0, 'Z'}, {1, 'Z'}}).add(a[1], {{0, 'X'}, {7, 'Y'}}).add(a[2], {{2, 'Y'}});
        seq.add(a[3], {{3, 'Z'}}).add(a[4], {{4, 'Z'}, {5, 'Z'}, {6, 'Z'}});
        seq.add(a[5], {{1, 'X'}, {2, 'X'}, {3, 'Y'}, {4, 'Z'}, {5, 'X'}, {6, 'Y'}}).add(a[6], {{7, 'Z'}});
        return seq;
    };
    const qsim::Circuit prep = qsim::createRandomCircuit(n, 60, 5);
    qsim::Simulator sim(n), plain(n);
    sim.run(prep);
    plain.run(prep);
    const qsim::Gradient g = sim.pauliGradient(sequence(angles), h);
    plain.applyPauliRotations(sequence(angles));
    ASSERT_TRUE(g.gradient.size() == angles.size());
    EXPECT_NEAR(g.value, plain.expectation(h), 0.0);
    EXPECT_NEAR(sim.state().maxAbsDiff(plain.state()), 0.0, 0.0);
    for (size_t k = 0; k < angles.size(); ++k) {
        double e[2];
        for (int side = 0; side < 2; ++side) {
            std::vector<double> shifted = angles;
            shifted[k] += side == 0 ? M_PI / 2 : -M_PI / 2;
            qsim::Simulator s(n);
            s.run(prep);
            s.applyPauliRotations(sequence(shifted));
            e[side] = s.expectation(h);
        }
        EXPECT_NEAR(g.gradient[k], (e[0] - e[1]) / 2, 1e-12 * abs_sum);
    }
    sim.releaseGradientBuffers();
}

TEST(PauliRotation, Exceptions) {
    qsim::Simulator sim(4);
    qsim::PauliSum h4(4), s4(4), s5(5);
    h4.add(1.0, {{0, 'Z'}});
    s4.add(0.3, {{1, 'X'}});
    s5.add(0.3, {{1, 'X'}});
    EXPECT_THROW(sim.applyPauliRotation({{4, 'X'}}, 0.3), std::out_of_range);
    EXPECT_THROW(sim.state().applyPauliRotation({{-1, 'Z'}}, 0.3), std::out_of_range);
    EXPECT_THROW(sim.applyPauliRotations(s5), std::invalid_argument);
    EXPECT_THROW(sim.state().applyPauliRotations(s5), std::invalid_argument);
    EXPECT_THROW(sim.pauliGradient(s5, h4), std::invalid_argument);
    EXPECT_THROW(sim.pauliGradient(s4, qsim::PauliSum(5)), std::invalid_argument);
    // nothing was applied: still |0000>
    const std::vector<cplx> psi = sim.getStateVector();
    EXPECT_NEAR(psi[0].real(), 1.0, 0.0);
    const qsim::Gradient none = sim.pauliGradient(s4, qsim::PauliSum(4));  // no terms: zeros
    EXPECT_NEAR(none.value, 0.0, 0.0);
    ASSERT_TRUE(none.gradient.size() == 1);
    EXPECT_NEAR(none.gradient[0], 0.0, 0.0);
    const qsim::Gradient empty = sim.pauliGradient(qsim::PauliSum(4), h4);  // no rotation: <H> as it is
    EXPECT_EQ(empty.gradient.size(), (size_t)0);
    EXPECT_NEAR(empty.value, sim.expectation(h4), 0.0);
}

TH_MAIN
