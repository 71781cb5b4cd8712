// test_dm_marginal.cpp — marginalProbabilities / reducedDensityMatrix / subsystemPurity /
// subsystemEntropy / fidelity of DensityMatrix and DensityMatrixSimulator through the C++17 layer
// (include/qsim/DensityMatrix.hpp) on a fixed 6-qubit noisy case, against plain loops over
// getDensityMatrix(); the exception types.
//
// Tolerance: a fixed-order sum of T terms of weight W = sum |terms| stays within 4 T 2^-52 W of the
// exact sum (the bound of tests/test_dm_marginal_gpu.py); W is accumulated beside each expected value.
#include <qsim/Circuit.hpp>
#include <qsim/DensityMatrix.hpp>
#include <qsim/NoiseModel.hpp>
#include <qsim/StateVector.hpp>

#include <cmath>
#include <complex>
#include <stdexcept>
#include <vector>

#include "harness.hpp"

using cd = std::complex<double>;
static const double kU = std::ldexp(1.0, -52);
static const int kN = 6;

static qsim::DensityMatrixSimulator noisy_case() {
    qsim::NoiseModel noise;
    noise.addDepolarizing(0.03);
    noise.addAmplitudeDamping({1}, 0.1);
    noise.addPhaseDamping({4}, 0.2);
    qsim::DensityMatrixSimulator sim(kN, noise);
    qsim::Circuit c(kN);
    c.h(0).cnot(0, 1).ry(2, 0.4).rx(3, 1.1).cz(2, 3).s(1).h(4).cnot(4, 2).t(5).h(5).cnot(5, 0).rz(3, 0.7).cnot(1, 4);
    sim.run(c);
    return sim;
}

// index of the n-qubit basis state whose bit qubits[j] is bit j of a and whose other bits are b's
static size_t compose(const std::vector<int>& qubits, size_t a, size_t b) {
    size_t i = 0;
    std::vector<bool> listed(kN, false);
    for (size_t j = 0; j < qubits.size(); ++j) {
        listed[qubits[j]] = true;
        if (a >> j & 1) i |= size_t(1) << qubits[j];
    }
    for (int q = 0, r = 0; q < kN; ++q)
        if (!listed[q]) {
            if (b >> r & 1) i |= size_t(1) << q;
            ++r;
        }
    return i;
}

TEST(DmMarginal, AgainstTheFullMatrix) {
    qsim::DensityMatrixSimulator sim = noisy_case();
    const size_t d = size_t(1) << kN;
    const std::vector<std::vector<int>> subsets = {{}, {0}, {5}, {3, 1}, {4, 0, 2}, {5, 4, 3, 2, 1, 0}, {2, 5, 0, 1, 3, 4}};
    std::vector<std::vector<double>> margs;
    std::vector<std::vector<cd>> mats;
    std::vector<double> purities, entropies, renyis;
    for (const auto& qs : subsets) {  // every reader first: they read rho where the run left it
        margs.push_back(sim.marginalProbabilities(qs));
        mats.push_back(sim.reducedDensityMatrix(qs));
        purities.push_back(sim.subsystemPurity(qs));
        entropies.push_back(sim.subsystemEntropy(qs));
        renyis.push_back(sim.subsystemEntropy(qs, true));
    }
    std::vector<cd> psi(d);
    for (size_t i = 0; i < d; ++i) psi[i] = cd(std::cos(0.37 * (double)i), std::sin(1.3 * (double)i) - 0.2);
    const double fid = sim.fidelity(psi);
    EXPECT_NEAR(sim.density().fidelity(psi), fid, 0.0);  // the same reduction: bitwise equal
    const std::vector<cd> m = sim.getDensityMatrix();
    for (size_t s = 0; s < subsets.size(); ++s) {
        const auto& qs = subsets[s];
        const size_t k = qs.size(), da = size_t(1) << k, nb = size_t(1) << (kN - k);
        EXPECT_EQ(margs[s].size(), da);
        EXPECT_EQ(mats[s].size(), da * da);
        double pur = 0.0;
        std::vector<cd> herm(da * da);
        for (size_t a = 0; a < da; ++a) {
            double p = 0.0, pw = 0.0;
            for (size_t b = 0; b < nb; ++b) {
                const size_t i = compose(qs, a, b);
                p += m[i * d + i].real();
                pw += std::abs(m[i * d + i].real());
            }
            EXPECT_NEAR(margs[s][a], p, 4.0 * (double)nb * kU * pw);
            for (size_t a2 = 0; a2 < da; ++a2) {
                cd v = 0.0;
                double w = 0.0;
                for (size_t b = 0; b < nb; ++b) {
                    const cd e = m[compose(qs, a, b) * d + compose(qs, a2, b)];
                    v += e;
                    w += std::abs(e);
                }
                EXPECT_NEAR(mats[s][a * da + a2].real(), v.real(), 4.0 * (double)nb * kU * w);
                EXPECT_NEAR(mats[s][a * da + a2].imag(), v.imag(), 4.0 * (double)nb * kU * w);
                pur += std::norm(mats[s][a * da + a2]);
            }
        }
        for (size_t a = 0; a < da; ++a)
            for (size_t a2 = 0; a2 < da; ++a2) herm[a * da + a2] = 0.5 * (mats[s][a * da + a2] + std::conj(mats[s][a2 * da + a]));
        EXPECT_NEAR(purities[s], pur, 0.0);  // the same host sum over the same matrix
        EXPECT_NEAR(renyis[s], -std::log2(pur), 1e-12);
        EXPECT_NEAR(entropies[s], qsim::hermitianEntropy(herm, (int)da), 0.0);
        EXPECT_NEAR(sim.density().subsystemEntropy(qs), entropies[s], 0.0);
    }
    // all qubits in order: the matrix itself and its diagonal, element for element
    const std::vector<int> all = {0, 1, 2, 3, 4, 5};
    const std::vector<cd> whole = sim.reducedDensityMatrix(all);
    const std::vector<double> diag = sim.marginalProbabilities(all), probs = sim.getProbabilities();
    for (size_t i = 0; i < d * d; ++i) EXPECT_TRUE(whole[i] == m[i]);
    for (size_t i = 0; i < d; ++i) EXPECT_TRUE(diag[i] == probs[i]);
    EXPECT_NEAR(sim.subsystemPurity(all), sim.getPurity(), 4.0 * (double)(d * d) * kU * sim.getPurity());
    cd f = 0.0;
    double fw = 0.0;
    for (size_t i = 0; i < d; ++i)
        for (size_t j = 0; j < d; ++j) {
            f += std::conj(psi[i]) * m[i * d + j] * psi[j];
            fw += std::abs(psi[i]) * std::abs(m[i * d + j]) * std::abs(psi[j]);
        }
    EXPECT_NEAR(fid, f.real(), 4.0 * (double)(d * d) * kU * fw);
    EXPECT_NEAR(sim.fidelity(psi), f.real(), 4.0 * (double)(d * d) * kU * fw);  // identity layout now
}

TEST(DmMarginal, PhysicsAnchors) {
    qsim::DensityMatrix mixed(kN);
    mixed.initMaximallyMixed();
    const std::vector<int> qs = {4, 1, 3};
    for (double p : mixed.marginalProbabilities(qs)) EXPECT_NEAR(p, 0.125, 1e-15);
    EXPECT_NEAR(mixed.subsystemEntropy(qs), 3.0, 1e-10);
    EXPECT_NEAR(mixed.subsystemPurity(qs), 0.125, 1e-15);
    std::vector<cd> bell(4, cd(0.0));
    bell[0] = bell[3] = std::sqrt(0.5);
    qsim::DensityMatrix rho(2, bell);
    EXPECT_NEAR(rho.fidelity(bell), 1.0, 1e-14);
    EXPECT_NEAR(rho.subsystemEntropy({0}), 1.0, 1e-10);
    EXPECT_NEAR(rho.subsystemEntropy({0, 1}), 0.0, 1e-10);
    std::vector<cd> e1(4, cd(0.0));
    e1[1] = 1.0;
    EXPECT_NEAR(rho.fidelity(e1), 0.0, 0.0);
}

TEST(DmMarginal, Exceptions) {
    qsim::DensityMatrixSimulator sim(5);
    qsim::DensityMatrix rho(3);
    EXPECT_THROW(sim.marginalProbabilities({1, 2, 1}), std::invalid_argument);
    EXPECT_THROW(sim.reducedDensityMatrix({0, 0}), std::invalid_argument);
    EXPECT_THROW(sim.marginalProbabilities({0, 5}), std::out_of_range);
    EXPECT_THROW(sim.reducedDensityMatrix({-1}), std::out_of_range);
    EXPECT_THROW(sim.subsystemPurity({4, 7}), std::out_of_range);
    EXPECT_THROW(rho.reducedDensityMatrix({0, 1, 2, 3}), std::invalid_argument);      // k > n
    EXPECT_THROW(rho.marginalProbabilities({0, 1, 2, 0}), std::invalid_argument);     // k > n
    qsim::DensityMatrix big(8);
    EXPECT_THROW(big.reducedDensityMatrix({0, 1, 2, 3, 4, 5, 6}), std::invalid_argument);  // k > 6
    EXPECT_THROW(big.subsystemEntropy({0, 1, 2, 3, 4, 5, 6}), std::invalid_argument);
    EXPECT_THROW(rho.fidelity(std::vector<cd>(4)), std::invalid_argument);
    EXPECT_THROW(sim.fidelity(std::vector<cd>(33)), std::invalid_argument);
    EXPECT_NO_THROW(rho.marginalProbabilities({2, 0, 1}));
}

TH_MAIN
