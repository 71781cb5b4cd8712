// C++ tests of the marginal-probability and reduced-density-matrix readout of the C++17 API
// (qsim::Simulator::marginalProbabilities / reducedDensityMatrix / subsystemPurity /
// entanglementEntropy).  Usage: test_marginal [--entropy=VALUE]: VALUE is the entropy the Python
// layer (numpy.linalg.eigvalsh) gets for the 12-qubit case below; the host's Jacobi sweep must
// agree with it to 1e-10.
#include <qsim/Circuit.hpp>
#include <qsim/NoiseModel.hpp>
#include <qsim/Simulator.hpp>
#include <qsim/StateVector.hpp>

#include <cmath>
#include <complex>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#include "harness.hpp"

using cplx = std::complex<double>;

static bool g_have_entropy = false;
static double g_entropy = 0.0;

TEST(Marginal, Bell) {
    qsim::Simulator sim(2);
    sim.run(qsim::createBellCircuit());
    for (int q = 0; q < 2; ++q) {
        const std::vector<double> m = sim.marginalProbabilities({q});
        ASSERT_TRUE(m.size() == 2);
        EXPECT_NEAR(m[0], 0.5, 1e-12);
        EXPECT_NEAR(m[1], 0.5, 1e-12);
        const std::vector<cplx> rho = sim.reducedDensityMatrix({q});
        ASSERT_TRUE(rho.size() == 4);
        EXPECT_NEAR(rho[0].real(), 0.5, 1e-12);
        EXPECT_NEAR(rho[3].real(), 0.5, 1e-12);
        EXPECT_NEAR(std::abs(rho[1]), 0.0, 1e-12);
        EXPECT_TRUE(rho[1] == std::conj(rho[2]));
        EXPECT_NEAR(sim.entanglementEntropy({q}), 1.0, 1e-10);
        EXPECT_NEAR(sim.entanglementEntropy({q}, true), 1.0, 1e-10);
        EXPECT_NEAR(sim.subsystemPurity({q}), 0.5, 1e-12);
    }
    EXPECT_NEAR(sim.marginalProbabilities({})[0], 1.0, 1e-12);
    EXPECT_NEAR(sim.state().entanglementEntropy({0, 1}), 0.0, 1e-10);
}

TEST(Marginal, GHZ) {
    qsim::Simulator sim(3);
    sim.run(qsim::createGHZCircuit(3));
    const std::vector<double> m = sim.marginalProbabilities({0, 2});
    ASSERT_TRUE(m.size() == 4);
    EXPECT_NEAR(m[0], 0.5, 1e-12);
    EXPECT_NEAR(m[1], 0.0, 1e-12);
    EXPECT_NEAR(m[2], 0.0, 1e-12);
    EXPECT_NEAR(m[3], 0.5, 1e-12);
    for (int q = 0; q < 3; ++q) EXPECT_NEAR(sim.entanglementEntropy({q}), 1.0, 1e-10);
    qsim::NoisySimulator noisy(3);
    noisy.run(qsim::createGHZCircuit(3));
    EXPECT_NEAR(noisy.marginalProbabilities({2, 1})[3], 0.5, 1e-12);
    EXPECT_NEAR(noisy.entanglementEntropy({1}), 1.0, 1e-10);
    EXPECT_NEAR(noisy.subsystemPurity({1}), 0.5, 1e-12);
    EXPECT_TRUE(noisy.reducedDensityMatrix({0, 1}).size() == 16);
}

TEST(Marginal, Exceptions) {
    qsim::Simulator sim(5);
    EXPECT_THROW(sim.marginalProbabilities({1, 3, 1}), std::invalid_argument);
    EXPECT_THROW(sim.reducedDensityMatrix({2, 2}), std::invalid_argument);
    EXPECT_THROW(sim.marginalProbabilities({0, 5}), std::out_of_range);
    EXPECT_THROW(sim.reducedDensityMatrix({-1}), std::out_of_range);
    EXPECT_THROW(sim.entanglementEntropy({0, 5}), std::out_of_range);
    EXPECT_THROW(sim.subsystemPurity({4, 4}), std::invalid_argument);
    EXPECT_NO_THROW(sim.marginalProbabilities({4, 0}));
}

TEST(Marginal, JacobiEntropy12) {
    qsim::Simulator sim(12);
    sim.run(qsim::createRandomCircuit(12, 120, 31));
    const std::vector<int> qubits = {0, 2, 5, 7, 8, 11};
    const std::vector<cplx> rho = sim.reducedDensityMatrix(qubits);
    ASSERT_TRUE(rho.size() == 64 * 64);
    double tr = 0.0;
    for (int i = 0; i < 64; ++i) tr += rho[i * 64 + i].real();
    EXPECT_NEAR(tr, 1.0, 1e-12);
    const std::vector<double> ev = qsim::hermitianEigenvalues(rho, 64);
    double sum = 0.0;
    for (double l : ev) sum += l;
    EXPECT_NEAR(sum, 1.0, 1e-12);
    EXPECT_TRUE(ev.front() > -1e-12);
    const double h = sim.entanglementEntropy(qubits);
    std::printf("Jacobi entropy of the 12-qubit case: %.17g\n", h);
    EXPECT_TRUE(h > 0.0 && h <= 6.0 + 1e-10);
    if (g_have_entropy) EXPECT_NEAR(h, g_entropy, 1e-10);
}

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        const std::string arg = argv[i];
        if (arg.rfind("--entropy=", 0) == 0) {
            g_entropy = std::strtod(arg.c_str() + 10, nullptr);
            g_have_entropy = true;
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
