// C++ tests of the marginal readout of qsim::DistributedSimulator
// (marginalProbabilities / reducedDensityMatrix / subsystemPurity / entanglementEntropy) on 8
// virtual ranks.  Usage: test_dist_marginal [--entropy=V] [--purity=V] [--marginal=V,V,...]: the
// values the Python layer gets on a sharded state for the 12-qubit case below (the entropy by
// numpy.linalg.eigvalsh); the host's Jacobi sweep must agree with the entropy to 1e-10, the rest
// to 1e-12.
#include <qsim/Circuit.hpp>
#include <qsim/DistributedSimulator.hpp>
#include <qsim/Simulator.hpp>
#include <qsim/StateVector.hpp>

#include <cmath>
#include <complex>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "harness.hpp"

using cplx = std::complex<double>;

static bool g_have_entropy = false, g_have_purity = false;
static double g_entropy = 0.0, g_purity = 0.0;
static std::vector<double> g_marginal;

TEST(DistMarginal, GhzKnownAnswers) {
    const int n = 12;
    qsim::DistributedSimulator d = qsim::DistributedSimulator::makeVirtual(n, 8);
    d.run(qsim::createGHZCircuit(n));
    // qubits on local and on rank positions alike
    for (const std::vector<int>& qs : {std::vector<int>{0, 11}, {11, 10, 9}, {3, 7}, {10}}) {
        const std::vector<double> m = d.marginalProbabilities(qs);
        ASSERT_TRUE(m.size() == (size_t(1) << qs.size()));
        EXPECT_NEAR(m.front(), 0.5, 1e-12);
        EXPECT_NEAR(m.back(), 0.5, 1e-12);
        for (size_t i = 1; i + 1 < m.size(); ++i) EXPECT_NEAR(m[i], 0.0, 1e-12);
        const std::vector<cplx> rho = d.reducedDensityMatrix(qs);
        const size_t D = m.size();
        ASSERT_TRUE(rho.size() == D * D);
        for (size_t r = 0; r < D; ++r)
            for (size_t c = 0; c < D; ++c) {
                EXPECT_NEAR(std::abs(rho[r * D + c] - cplx(r == c ? m[r] : 0.0)), 0.0, 1e-12);
                EXPECT_TRUE(rho[r * D + c] == std::conj(rho[c * D + r]));
            }
        EXPECT_NEAR(d.subsystemPurity(qs), 0.5, 1e-12);
        EXPECT_NEAR(d.entanglementEntropy(qs), 1.0, 1e-10);
        EXPECT_NEAR(d.entanglementEntropy(qs, true), 1.0, 1e-10);
    }
    EXPECT_NEAR(d.marginalProbabilities({})[0], 1.0, 1e-12);
}

TEST(DistMarginal, MatchesSimulator) {
    const int n = 12;
    const qsim::Circuit c = qsim::createRandomHCCircuit(n, 100, 42);
    qsim::DistributedSimulator d = qsim::DistributedSimulator::makeVirtual(n, 8);
    qsim::Simulator sim(n);
    for (int rep = 0; rep < 3; ++rep) {
        d.run(c);
        sim.run(c);
    }
    const std::vector<cplx> before = d.getStateVector();
    for (const std::vector<int>& qs : {std::vector<int>{0, 1, 2}, {11, 4}, {9, 10, 11}, {5, 0, 11, 7, 2, 9}, {}}) {
        const std::vector<double> m = d.marginalProbabilities(qs), ms = sim.marginalProbabilities(qs);
        ASSERT_TRUE(m.size() == ms.size());
        for (size_t i = 0; i < m.size(); ++i) EXPECT_NEAR(m[i], ms[i], 1e-12);
        const std::vector<cplx> rho = d.reducedDensityMatrix(qs), rs = sim.reducedDensityMatrix(qs);
        ASSERT_TRUE(rho.size() == rs.size());
        for (size_t i = 0; i < rho.size(); ++i) EXPECT_NEAR(std::abs(rho[i] - rs[i]), 0.0, 1e-12);
        EXPECT_TRUE(d.reducedDensityMatrix(qs) == rho);  // fixed-order sums: bit for bit
        EXPECT_TRUE(d.marginalProbabilities(qs) == m);
    }
    EXPECT_TRUE(d.getStateVector() == before);
}

TEST(DistMarginal, Exceptions) {
    qsim::DistributedSimulator d = qsim::DistributedSimulator::makeVirtual(12, 8);
    EXPECT_THROW(d.marginalProbabilities({1, 3, 1}), std::invalid_argument);
    EXPECT_THROW(d.reducedDensityMatrix({2, 2}), std::invalid_argument);
    EXPECT_THROW(d.marginalProbabilities({0, 12}), std::out_of_range);
    EXPECT_THROW(d.reducedDensityMatrix({-1}), std::out_of_range);
    EXPECT_THROW(d.entanglementEntropy({0, 12}), std::out_of_range);
    EXPECT_THROW(d.subsystemPurity({4, 4}), std::invalid_argument);
    EXPECT_THROW(d.reducedDensityMatrix({0, 1, 2, 3, 4, 5, 6}), std::invalid_argument);
    EXPECT_NO_THROW(d.marginalProbabilities({11, 0}));
}

// marginal_cases.CPP_ENTROPY_CASE on a sharded state
TEST(DistMarginal, JacobiEntropy12) {
    qsim::DistributedSimulator d = qsim::DistributedSimulator::makeVirtual(12, 8);
    d.run(qsim::createRandomCircuit(12, 120, 31));
    const std::vector<int> qubits = {0, 2, 5, 7, 8, 11};
    const std::vector<cplx> rho = d.reducedDensityMatrix(qubits);
    ASSERT_TRUE(rho.size() == 64 * 64);
    double tr = 0.0;
    for (int i = 0; i < 64; ++i) tr += rho[i * 64 + i].real();
    EXPECT_NEAR(tr, 1.0, 1e-12);
    const std::vector<double> ev = qsim::hermitianEigenvalues(rho, 64);
    EXPECT_TRUE(ev.front() > -1e-12);
    const double h = d.entanglementEntropy(qubits);
    std::printf("Jacobi entropy of the sharded 12-qubit case: %.17g\n", h);
    EXPECT_TRUE(h > 0.0 && h <= 6.0 + 1e-10);
    if (g_have_entropy) EXPECT_NEAR(h, g_entropy, 1e-10);
    if (g_have_purity) EXPECT_NEAR(d.subsystemPurity(qubits), g_purity, 1e-12);
    if (!g_marginal.empty()) {
        const std::vector<double> m = d.marginalProbabilities({11, 3});
        ASSERT_TRUE(m.size() == g_marginal.size());
        for (size_t i = 0; i < m.size(); ++i) EXPECT_NEAR(m[i], g_marginal[i], 1e-12);
    }
}

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        const std::string arg = argv[i];
        if (arg.rfind("--entropy=", 0) == 0) {
            g_entropy = std::strtod(arg.c_str() + 10, nullptr);
            g_have_entropy = true;
        } else if (arg.rfind("--purity=", 0) == 0) {
            g_purity = std::strtod(arg.c_str() + 9, nullptr);
            g_have_purity = true;
        } else if (arg.rfind("--marginal=", 0) == 0) {
            const char* p = arg.c_str() + 11;
            while (*p) {
                char* end = nullptr;
                g_marginal.push_back(std::strtod(p, &end));
                p = *end == ',' ? end + 1 : end;
            }
        }
    }
    int failed_cases = 0, run = 0;
    for (const th::Case& c : th::registry()) {
        const std::string id = std::string(c.suite) + "." + c.name;
        const int before = th::failures();
        ++run;
        try {
            c.fn();
        } catch (const th::Abort&) {
        } catch (const std::exception& e) {
            th::fail(__FILE__, __LINE__, std::string("uncaught: ") + e.what());
        }
        const bool ok = th::failures() == before;
        if (!ok) ++failed_cases;
        std::printf("[%s] %s\n", ok ? "  OK  " : " FAIL ", id.c_str());
    }
    std::printf("%d cases, %d failed\n", run, failed_cases);
    return failed_cases;
}
