// The bin of a dose, written once for exposure_absorb_kernel (cpf_exposure.hip) and for cpf_exposure_bins_host (cpf_ledger.cpp):
//   k = dose * invWidth, invWidth = 1.0 / binWidth computed once on the host; bin = k >= nBins - 1 ? nBins - 1 : (int)k.
// Each operation is rounded on its own (the library is built with -ffp-contract=off, and there is nothing here to contract).
// The last bin is open-ended: an infinite dose lands there.  A dose the accumulate rule cannot produce -- negative, or NaN -- has
// no bin: -1, and the kernel counts no such particle (cpf_exposure_set_doses refuses these values).
#pragma once
#include <hip/hip_runtime.h>

namespace cpf {

__host__ __device__ __forceinline__ int exposure_bin(double dose, double invWidth, int nBins) {
    const double k = dose * invWidth;
    if (!(k >= 0.0)) return -1;
    return k >= (double)(nBins - 1) ? nBins - 1 : (int)k;
}

}  // namespace cpf
