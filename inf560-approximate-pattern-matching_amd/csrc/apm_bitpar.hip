/*
 * apm_bitpar.hip -- the BITPAR launcher and the kernel for patterns of up to 128 bytes (bit-vector columns of 1..4 words).
 * The kernel's body lives in apm_bitpar.h; the wider columns are units of their own (apm_bitpar_wide.hip, apm_bitlong.hip),
 * which this launcher hands longer patterns to.
 */
#include "apm_internal.h"
#include "apm_core.h"
#include "apm_bitpar.h"

size_t apm_bitpar_lds_bytes(const ApmScanArgs &a) {
    const size_t tile_bytes = (size_t)((a.tile + a.halo + APM_TILE_SLACK + 15) & ~15);
    return tile_bytes + 256 + (size_t)((a.table_words + 3) & ~3) * 4 + (size_t)a.n_pats * 4 + 16;
}

hipError_t apm_launch_bitpar(const ApmScanArgs &a, hipStream_t s) {
    const int64_t span = a.je - a.tile0;
    if (span <= 0 || a.n_pats <= 0) return hipSuccess;
    const int64_t nt = (span + a.tile - 1) / a.tile;
    if (nt > 0x7fffffffLL) return hipErrorInvalidValue;
    if (a.halo >= 512) return apm_launch_bitpar_xwide(a, (unsigned)nt, apm_bitpar_lds_bytes(a), s); // 513 .. 1024 bytes (apm_bitlong.hip)
    if (a.halo >= 128) return apm_launch_bitpar_wide(a, (unsigned)nt, apm_bitpar_lds_bytes(a), s); // (the runtime never mixes; apm_bitpar_wide.hip)
    hipLaunchKernelGGL(apm_bitpar_kernel<false>, dim3((unsigned)nt), dim3(APM_BLOCK), apm_bitpar_lds_bytes(a), s, a);
    return hipGetLastError();
}
