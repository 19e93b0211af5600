/*
 * apm_sieve_diag.hip -- the code-filter SIEVE with the DIAGONAL form of its window DP on codes (k <= 3): the kernel
 * apm_sieve2cfdp_kernel of apm_sieve.hip with apm_code_dp_diag (apm_core.h) in place of the column loop and the region
 * trimmed to what the verify launch can reach, [s - off - k / 2, s - off + m + k / 2).  The column form pays m + 2k
 * columns for every queue entry, whatever the outcome; this one pays eight furthest-reaching steps per window start.
 * A unit of its own: the registers and the LDS of the kernels in apm_sieve.hip are pinned (tests/test_verify_resources.py).
 * Launched by apm_launch_sieve2 (apm_sieve.hip) with the column kernel's geometry rules, LDS layout and arguments.
 */
#include "apm_sieve_body.h"

__global__ __launch_bounds__(1024, 8) void apm_sieve2cfdg_kernel(ApmSieve2PoolArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    apm_sieve2_body<true, true, true, ApmSieve2PoolArgs>(a, smem);
}

// (the launcher lives in the other unit: it asks for the kernel here)
const void *apm_sieve2cfdg_fn() { return (const void *)apm_sieve2cfdg_kernel; }
