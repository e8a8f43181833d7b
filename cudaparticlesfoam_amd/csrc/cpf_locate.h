// The initial-locate rule as a device function: locate_initial_kernel (cpf_kernels.hip) and the respawn kernel (cpf_recycle.hip)
// give a point the same cell.
#pragma once
#include "cpf_walk.h"        // D3, plane_dist

namespace cpf {

// bin grid + point-in-convex-cell plane test (replaces OptiX query + baryQuery, query/RTQuery.cu:295-310): the lowest-numbered
// cell whose every plane has P on its inner side (bins list cells ascending), else CPF_CELL_LOST
// (cellOff, planes: MeshView's)
__device__ __forceinline__ int locate_point(const D3& P, const int32_t* __restrict__ cellOff, const double4* __restrict__ planes,
                                             const GridView& g) {
    int found = CPF_CELL_LOST;
    const bool inBox = P.x >= g.lo[0] && P.x <= g.hi[0] && P.y >= g.lo[1] && P.y <= g.hi[1] && P.z >= g.lo[2] &&
                       P.z <= g.hi[2];
    if (inBox) {
        int b[3];
        const double pv[3] = {P.x, P.y, P.z};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            long long q = (long long)floor((pv[k] - g.origin[k]) * g.invBin[k]);
            q = q < 0 ? 0 : (q > g.dims[k] - 1 ? g.dims[k] - 1 : q);
            b[k] = (int)q;
        }
        const int64_t bin = ((int64_t)b[2] * g.dims[1] + b[1]) * g.dims[0] + b[0];
        for (int k = g.binOff[bin]; k < g.binOff[bin + 1] && found < 0; ++k) {
            const int c = g.binCells[k];
            bool inside = true;
            for (int s = cellOff[c]; s < cellOff[c + 1]; ++s) {
                const double4 pl = planes[s];
                if (!(plane_dist(pl, P) <= 0.0)) { inside = false; break; }
            }
            if (inside) found = c;
        }
    }
    return found;
}

}  // namespace cpf
