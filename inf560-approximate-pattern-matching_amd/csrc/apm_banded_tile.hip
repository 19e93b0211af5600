/*
 * apm_banded_tile.hip -- launcher of the LDS-tile BANDED kernel (apm_banded_tile.h).  The kernel itself is instantiated
 * band by band in apm_banded_tile_b0.hip .. _b3.hip; this unit asks them for the kernel of a launch.
 */
#include "apm_internal.h"

size_t apm_filter_lds_bytes(const ApmFilterArgs &a) { // always >= 4352 B, which the tail workgroups need
    return (size_t)(a.use_dma ? (a.stride == 1 ? 4 : 3) : 2) * (size_t)a.tile_len + (size_t)a.image_len + 2 * (size_t)a.qcap * 4 +
           (size_t)((a.n_pats + 3) & ~3) * 4 + 32 + 4 * 128 * 4 + 16; // counters [8] + 4 survivor lists (SCAP = 128)
}

/* the kernel for (kl, stride, dma) out of the unit of each band; nullptr if there is none */
const void *apm_filter_fn_b0(int kl, int stride, int dma);
const void *apm_filter_fn_b1(int kl, int stride, int dma);
const void *apm_filter_fn_b2(int kl, int stride, int dma);
const void *apm_filter_fn_b3(int kl, int stride, int dma);

static const void *apm_filter_fn(int band, int kl, int stride, int dma) {
    switch (band) {
    case 0: return apm_filter_fn_b0(kl, stride, dma);
    case 1: return apm_filter_fn_b1(kl, stride, dma);
    case 2: return apm_filter_fn_b2(kl, stride, dma);
    case 3: return apm_filter_fn_b3(kl, stride, dma);
    default: return nullptr;
    }
}

// workgroups of the filter kernel resident per CU for this LDS budget (queried once per plan)
int apm_filter_blocks_per_cu(int band, int kl, int stride, int dma, size_t lds) {
    int per_cu = 0;
    const void *fn = apm_filter_fn(band, kl, stride, dma);
    if (!fn || hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, APM_BLOCK, lds) != hipSuccess || per_cu < 1) {
        (void)hipGetLastError();
        per_cu = 2;
    }
    return per_cu > 8 ? 8 : per_cu;
}

hipError_t apm_launch_filter(const ApmFilterArgs &a, int max_blocks, hipStream_t s) {
    if (a.ntiles <= 0 || a.n_pats <= 0) return hipSuccess;
    if (a.ntiles > ((int64_t)1 << 30)) return hipErrorInvalidValue; // 32-bit tile indices in the kernel
    const void *fn = apm_filter_fn(a.band, a.key_len, a.stride, a.use_dma);
    if (!fn) return hipErrorInvalidValue;
    const size_t lds = apm_filter_lds_bytes(a);
    const int64_t cap = max_blocks < 1 ? 1 : max_blocks; // persistent grid = resident workgroups
    const int64_t nb = a.ntiles < cap ? a.ntiles : cap;
    ApmFilterArgs args = a;
    args.n_main_blocks = (int)nb;
#ifdef APM_MEASURE
    if (const char *e = getenv("APM_MEASURE_SKIP")) args.skip_mask = atoi(e);
#endif
    void *kargs[] = {&args};
    return hipLaunchKernel(fn, dim3((unsigned)(nb + a.n_tail)), dim3(APM_BLOCK), kargs, lds, s);
}
