// Parent <-> derived cell ids of a mesh whose warped or concave cells were decomposed into tets (cpf_mesh.cpp, derive_mesh;
// DESIGN.md "Warped cells").  The walk runs on the derived cells; the caller's velocity field and every cell id it reads back
// are per PARENT cell.  Both maps are one gather per element: memory bound, no reuse, one thread each.
#include <hip/hip_runtime.h>

#include "cpf_device.h"

namespace cpf {
namespace {

constexpr int kParentBlock = 256;

inline dim3 parent_grid(int64_t n) { return dim3((unsigned)((n + kParentBlock - 1) / kParentBlock)); }

// U of derived cell d = U of its parent (the fan of a cell carries the cell's velocity, as the reference's 12 tets of a hex do:
// src/initCuda.H:106-108)
__global__ void __launch_bounds__(kParentBlock)
gather_parent_u3_kernel(const double* __restrict__ uParent, const int32_t* __restrict__ parentOf, double* __restrict__ uDerived,
                        int64_t nDerived) {
    const int64_t d = (int64_t)blockIdx.x * kParentBlock + threadIdx.x;
    if (d >= nDerived) return;
    const int64_t p = parentOf[d];
    uDerived[3 * d + 0] = uParent[3 * p + 0];
    uDerived[3 * d + 1] = uParent[3 * p + 1];
    uDerived[3 * d + 2] = uParent[3 * p + 2];
}

// derived -> parent id; negative codes (CPF_CELL_LOST, CPF_CELL_FROZEN) and ids beyond the mesh pass through unchanged
// (in and out may alias)
__global__ void __launch_bounds__(kParentBlock)
cells_to_parent_kernel(const int32_t* in, int32_t* out, const int32_t* __restrict__ parentOf, int64_t n, int64_t nDerived) {
    const int64_t i = (int64_t)blockIdx.x * kParentBlock + threadIdx.x;
    if (i >= n) return;
    const int32_t c = in[i];
    out[i] = (c >= 0 && c < nDerived) ? parentOf[c] : c;
}

}  // namespace

hipError_t launch_gather_parent_u3(hipStream_t st, const double* uParent, const int32_t* parentOf, double* uDerived,
                                   int64_t nDerived) {
    if (nDerived > 0)
        hipLaunchKernelGGL(gather_parent_u3_kernel, parent_grid(nDerived), dim3(kParentBlock), 0, st, uParent, parentOf, uDerived,
                           nDerived);
    return hipGetLastError();
}

hipError_t launch_cells_to_parent(hipStream_t st, const int32_t* in, int32_t* out, const int32_t* parentOf, int64_t n,
                                  int64_t nDerived) {
    if (n > 0)
        hipLaunchKernelGGL(cells_to_parent_kernel, parent_grid(n), dim3(kParentBlock), 0, st, in, out, parentOf, n, nDerived);
    return hipGetLastError();
}

}  // namespace cpf
