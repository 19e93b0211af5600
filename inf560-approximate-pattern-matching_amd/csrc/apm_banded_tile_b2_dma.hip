/*
 * apm_banded_tile_b2_dma.hip -- the LDS-tile BANDED kernel (apm_banded_tile.h) for band 2, LDS-DMA form: 5 key classes.
 * apm_banded_tile_b2.hip holds the band's getter and asks this unit for the DMA forms; the same rule holds for this
 * getter: an ordinary external function with a _rec rename in apm_rec.h.
 */
#include "apm_banded_tile.h"

const void *apm_filter_fn_b2_dma(int kl, int stride) {
    return apm_filter_fn_kl<2, 1>(kl, stride);
}
