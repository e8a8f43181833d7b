// TEST INFRASTRUCTURE ONLY: the walk's acceptance predicate (cudaparticlesfoam_amd/csrc/cpf_accept.h) built by the host
// compiler, over arrays, for tests/test_accept_predicate_host.py.  Every case is the FIRST face of a visit: no running
// minimum yet, and a token that matches no neighbour.
#include <cstdint>

#include "cpf_accept.h"

namespace {
constexpr int kToken = -7;
template <bool GROUPS>
void pruned(const double* den, const double* fd, int64_t n, int nb, uint8_t* out) {
    for (int64_t i = 0; i < n; ++i) {
        double dTmin = 2.0;
        int next = -1, best = -1;
        cpf::face_accept<GROUPS>(den[i], fd[i], nb, kToken, 0, dTmin, next, best);
        out[i] = best == 0;
    }
}
}  // namespace

extern "C" {
void accept_pruned(const double* den, const double* fd, int64_t n, int groups, int nb, uint8_t* out) {
    groups ? pruned<true>(den, fd, n, nb, out) : pruned<false>(den, fd, n, nb, out);
}
int accept_is_group(int nb) { return cpf::is_group(nb); }
double accept_tol() { return cpf::kTol; }
}
