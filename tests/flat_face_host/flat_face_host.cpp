// Host check of the chain form of the face acceptance (csrc/cpf_accept.h, face_accept_chain: what the hand-written face block of
// the flat walk executes) against face_accept<false>: accepted set, dTmin, next and best must be equal for every input.
// A plain executable (tests/test_flat_face_predicate_host.py builds and runs it); exit status 0 = equal everywhere, and the last
// line printed is "cases <n> accepted <m> mismatches 0".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "cpf_accept.h"

namespace {

uint64_t bits(double v) { uint64_t u; std::memcpy(&u, &v, 8); return u; }
double ulp_up(double v) { return std::nextafter(v, std::numeric_limits<double>::infinity()); }
double ulp_down(double v) { return std::nextafter(v, -std::numeric_limits<double>::infinity()); }

long long g_cases = 0, g_accepted = 0, g_bad = 0;

void one(double den, double fd, int bs, int token, double dTmin0) {
    double dA = dTmin0, dB = dTmin0;
    int nA = -7, nB = -7, bA = -1, bB = -1;
    cpf::face_accept<false>(den, fd, bs, token, 3, dA, nA, bA);
    cpf::face_accept_chain(den, fd, bs, token, 3, dB, nB, bB);
    ++g_cases;
    g_accepted += bA == 3;
    if (bits(dA) != bits(dB) || nA != nB || bA != bB) {
        if (g_bad++ < 20)
            std::printf("MISMATCH den %a fd %a bs %d token %d dTmin %a: accept (%a, %d, %d) chain (%a, %d, %d)\n", den, fd, bs, token,
                        dTmin0, dA, nA, bA, dB, nB, bB);
    }
}

void all_tokens(double den, double fd, double dTmin0) {
    one(den, fd, 11, 12, dTmin0);
    one(den, fd, 11, 11, dTmin0);          // bs == token: the entry face
    one(den, fd, -1, 12, dTmin0);          // a wall
}

}  // namespace

int main() {
    using lim = std::numeric_limits<double>;
    const double tol = cpf::kTol;
    std::vector<double> mags = {0.0, lim::denorm_min(), 2 * lim::denorm_min(), ulp_down(lim::min()), lim::min(), ulp_up(lim::min()),
                                1e-300, 1e-20, ulp_down(tol), tol, ulp_up(tol), 2 * tol, 1e-7, 0.25, 0.5, ulp_down(1.0), 1.0, ulp_up(1.0),
                                2.0, 3.0, 1e20, 1e300, ulp_down(lim::max()), lim::max(), lim::infinity()};
    std::vector<double> grid;
    for (double m : mags) { grid.push_back(m); grid.push_back(-m); }
    grid.push_back(lim::quiet_NaN());
    grid.push_back(-lim::quiet_NaN());
    const std::vector<double> mins = {2.0, 1.0, 0.5, ulp_up(tol), tol, 1e-300};
    // the grid: every pair (fd, den), |fd| == |den| included (the diagonal), fd at tol and one ulp either side
    for (double fd : grid)
        for (double den : grid)
            for (double m : mins) all_tokens(den, fd, m);
    // dT one ulp either side of tol and of dTmin: den a power of two (the quotient is exact), fd = den * target
    for (double den : {1.0, -1.0, 0.5, -0.5, 0x1p-20, -0x1p-20, 0x1p+10, -0x1p+10})
        for (double target : {ulp_down(tol), tol, ulp_up(tol), ulp_down(0.5), 0.5, ulp_up(0.5), ulp_down(1.0), 1.0, ulp_up(1.0)})
            for (double m : {2.0, 0.5, tol, ulp_up(tol), 1.0}) {
                all_tokens(den, den * target, m);
                all_tokens(den, -den * target, m);
                all_tokens(den, den * target, target);          // dT == dTmin: the strict "<" keeps the earlier face
            }
    // random pairs: magnitudes log-uniform over the exponent range that matters and over all of it, both signs, and near-equal pairs
    std::mt19937_64 rng(20240607);
    std::uniform_real_distribution<double> u01(0.0, 1.0);
    auto draw = [&](double lo10, double hi10) {
        const double m = std::pow(10.0, lo10 + (hi10 - lo10) * u01(rng));
        return (rng() & 1) ? m : -m;
    };
    for (int k = 0; k < 1000000; ++k) {
        double den, fd;
        switch (k % 4) {
            case 0: den = draw(-3, 1); fd = draw(-16, 1); break;
            case 1: den = draw(-300, 300); fd = draw(-300, 300); break;
            case 2: den = draw(-3, 1); fd = den * (1.0 + (u01(rng) - 0.5) * 1e-15 * (double)(rng() % 8)); if (rng() & 1) fd = -fd; break;
            default: den = draw(-12, 1); fd = draw(-16, -12); break;
        }
        const double m = (k % 3 == 0) ? 2.0 : u01(rng);
        one(den, fd, (int)(rng() % 5), (int)(rng() % 5), m);
    }
    std::printf("cases %lld accepted %lld mismatches %lld\n", g_cases, g_accepted, g_bad);
    return g_bad == 0 ? 0 : 1;
}
