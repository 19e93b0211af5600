/*
 * apm_banded_tile_b2.hip -- the LDS-tile BANDED kernel (apm_banded_tile.h) for band 2, the longest compile of the four:
 * this unit holds the 5 key classes of the register-staged form, apm_banded_tile_b2_dma.hip those of the LDS-DMA form.
 * The getter is an ordinary external function with a _rec rename in apm_rec.h (a template or an inline one would be weak,
 * and the linker would fold the record build's copy into the counting build's without a word).
 */
#include "apm_banded_tile.h"

const void *apm_filter_fn_b2_dma(int kl, int stride); /* apm_banded_tile_b2_dma.hip */

const void *apm_filter_fn_b2(int kl, int stride, int dma) {
    return dma ? apm_filter_fn_b2_dma(kl, stride) : apm_filter_fn_kl<2, 0>(kl, stride);
}
