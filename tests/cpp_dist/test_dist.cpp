// test_dist.cpp — qsim::DistributedSimulator (include/qsim/DistributedSimulator.hpp), the sharded
// engine behind Simulator's interface: 4 virtual ranks at 12 qubits against the parity oracle
// (oracle/cpu_simulator.hpp) — run, getProbabilities, sample under setSeed, measureQubit — and
// the exception types.
#include <qsim/Circuit.hpp>
#include <qsim/DistributedSimulator.hpp>
#include <qsim/Simulator.hpp>

#include <cmath>
#include <complex>
#include <stdexcept>
#include <vector>

#include "cpu_simulator.hpp"
#include "harness.hpp"

using cplx = std::complex<double>;

static double max_diff(const std::vector<cplx>& a, const std::vector<cplx>& b) {
    if (a.size() != b.size()) return 1e300;
    double m = 0.0;
    for (size_t i = 0; i < a.size(); ++i)
        m = std::fmax(m, std::fmax(std::fabs(a[i].real() - b[i].real()), std::fabs(a[i].imag() - b[i].imag())));
    return m;
}

TEST(Dist, RunAndProbabilitiesMatchOracle) {
    const int n = 12;
    const qsim::Circuit c = qsim::createRandomCircuit(n, 100, 5);
    qsim_oracle::CPUSimulator cpu(n);
    cpu.run(c);
    cpu.run(c);
    for (qsim::RunMode m : {qsim::RunMode::Fused, qsim::RunMode::PerGate}) {
        qsim::DistributedSimulator d = qsim::DistributedSimulator::makeVirtual(n, 4);
        EXPECT_EQ(d.getNumQubits(), n);
        EXPECT_EQ(d.getWorldSize(), 4);
        EXPECT_EQ(d.getRank(), 0);
        d.setRunMode(m);
        d.run(c);
        d.run(c);
        d.synchronize();
        EXPECT_NEAR(max_diff(d.getStateVector(), cpu.getStateVector()), 0.0, 1e-12);
        const std::vector<double> p = d.getProbabilities(), want = cpu.getProbabilities();
        ASSERT_TRUE(p.size() == want.size());
        double worst = 0.0;
        for (size_t i = 0; i < p.size(); ++i) worst = std::fmax(worst, std::fabs(p[i] - want[i]));
        EXPECT_NEAR(worst, 0.0, 1e-12);
    }
    // runSequence: the same gates as one sharded run; reset: back to |0..0>
    qsim::DistributedSimulator d = qsim::DistributedSimulator::makeVirtual(n, 4);
    d.runSequence({c, c});
    EXPECT_NEAR(max_diff(d.getStateVector(), cpu.getStateVector()), 0.0, 1e-12);
    d.reset();
    const std::vector<cplx> z = d.getStateVector();
    EXPECT_NEAR(std::abs(z[0] - cplx(1.0, 0.0)), 0.0, 0.0);
}

TEST(Dist, SampleUnderSeed) {
    const int n = 12, shots = 500;
    const qsim::Circuit c = qsim::createRandomHCCircuit(n, 100, 42);
    qsim_oracle::CPUSimulator cpu(n);
    cpu.run(c);
    cpu.run(c);
    const std::vector<double> p = cpu.getProbabilities();
    std::vector<std::vector<int>> got;
    for (int rep = 0; rep < 2; ++rep) {
        qsim::DistributedSimulator d = qsim::DistributedSimulator::makeVirtual(n, 4);
        d.run(c);
        d.run(c);
        d.setSeed(1234);
        got.push_back(d.sample(shots));
        ASSERT_TRUE(got.back().size() == (size_t)shots);
        for (int i : got.back()) {
            ASSERT_TRUE(i >= 0 && i < (1 << n));
            EXPECT_TRUE(p[i] > 0.0);
        }
        // sampling moved no amplitude
        EXPECT_NEAR(max_diff(d.getStateVector(), cpu.getStateVector()), 0.0, 1e-12);
        EXPECT_TRUE(d.sample(0).empty());
    }
    EXPECT_TRUE(got[0] == got[1]);  // the same seed: the same shots
    // the shots follow the distribution: the most likely outcome's count is within 6 sigma
    size_t top = 0;
    for (size_t i = 1; i < p.size(); ++i)
        if (p[i] > p[top]) top = i;
    int cnt = 0;
    for (int i : got[0]) cnt += (size_t)i == top;
    EXPECT_NEAR((double)cnt, shots * p[top], 6.0 * std::sqrt(shots * p[top] * (1.0 - p[top])) + 1.0);
}

TEST(Dist, MeasureQubit) {
    const int n = 12;
    const qsim::Circuit c = qsim::createRandomCircuit(n, 100, 5);
    for (int q : {0, 4, 11}) {
        qsim_oracle::CPUSimulator cpu(n);
        cpu.run(c);
        qsim::DistributedSimulator d = qsim::DistributedSimulator::makeVirtual(n, 4);
        d.run(c);
        d.setSeed(7 + q);
        const int bit = n - 1 - q;  // reference semantics (F2)
        const double p0 = cpu.probBitZero(bit);
        const int r = d.measureQubit(q);
        ASSERT_TRUE(r == 0 || r == 1);
        const double pr = r == 0 ? p0 : 1.0 - p0;
        ASSERT_TRUE(pr > 1e-15);
        cpu.collapse(bit, r, 1.0 / std::sqrt(pr));
        EXPECT_NEAR(max_diff(d.getStateVector(), cpu.getStateVector()), 0.0, 1e-12);
        double total = 0.0;
        for (double x : d.getProbabilities()) total += x;
        EXPECT_NEAR(total, 1.0, 1e-12);
        EXPECT_EQ(d.measureQubit(q), r);  // measured again: the same result
    }
}

TEST(Dist, Exceptions) {
    EXPECT_THROW(qsim::DistributedSimulator::makeVirtual(12, 3), std::invalid_argument);
    EXPECT_THROW(qsim::DistributedSimulator::makeVirtual(0, 1), std::invalid_argument);
    EXPECT_THROW(qsim::DistributedSimulator::makeVirtual(4, 16), std::invalid_argument);
    qsim::DistributedSimulator d = qsim::DistributedSimulator::makeVirtual(10, 4);
    EXPECT_THROW(d.run(qsim::Circuit(9)), std::invalid_argument);
    const std::vector<qsim::Circuit> mixed = {qsim::Circuit(10), qsim::Circuit(11)};
    EXPECT_THROW(d.runSequence(mixed), std::invalid_argument);
    EXPECT_THROW(d.measureQubit(-1), std::invalid_argument);
    EXPECT_THROW(d.measureQubit(10), std::invalid_argument);
    EXPECT_THROW(d.sample(-1), std::invalid_argument);
    EXPECT_NO_THROW(d.run(qsim::Circuit(10)));
    EXPECT_EQ(d.measureQubit(3), 0);  // |0..0>
    // moving keeps the engine object alive in exactly one owner
    qsim::DistributedSimulator e = std::move(d);
    EXPECT_EQ(e.getNumQubits(), 10);
    EXPECT_NEAR(e.getProbabilities()[0], 1.0, 1e-15);
}

TH_MAIN
