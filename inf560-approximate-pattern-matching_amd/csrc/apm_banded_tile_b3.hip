/*
 * apm_banded_tile_b3.hip -- the LDS-tile BANDED kernel (apm_banded_tile.h) for band 3: 5 key classes x 2 DMA forms.
 * The getter is an ordinary external function with a _rec rename in apm_rec.h (a template or an inline one would be weak,
 * and the linker would fold the record build's copy into the counting build's without a word).
 */
#include "apm_banded_tile.h"

const void *apm_filter_fn_b3(int kl, int stride, int dma) {
    return dma ? apm_filter_fn_kl<3, 1>(kl, stride) : apm_filter_fn_kl<3, 0>(kl, stride);
}
