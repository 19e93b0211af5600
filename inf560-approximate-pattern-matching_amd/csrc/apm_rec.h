/*
 * apm_rec.h -- the RECORD build of the kernel files.
 *
 * The Makefile compiles every kernel file twice: as it stands (the counting kernels, whose registers, LDS and
 * occupancy are tuned and must not move) and with -DAPM_REC into csrc/<file>_rec.o.  In the record build every place
 * that decides a matching (pattern, window) pair also appends a 16-byte record {pos, pattern, 0} to the sink of the
 * launch (ApmPosSink in apm_internal.h): the kernels behind apm_find_all_buffer and apm_find_shard_device.  Everything
 * else is the same source, so the two builds cannot drift apart.  The record build's kernels and launchers carry the
 * suffix _rec -- this header renames them, nothing more; the runtime (compiled once, without APM_REC) picks
 * apm_launch_x or apm_launch_x_rec per call.
 */
#ifndef APM_REC_H
#define APM_REC_H
#ifdef APM_REC
/* kernels */
#define apm_bitpar_kernel apm_bitpar_kernel_rec
#define apm_bitpar_xwide_kernel apm_bitpar_xwide_kernel_rec
#define apm_bitlong_kernel apm_bitlong_kernel_rec
#define apm_wavefront_kernel apm_wavefront_kernel_rec
#define apm_generic_kernel apm_generic_kernel_rec
#define apm_nfa_kernel apm_nfa_kernel_rec
#define apm_tail_kernel apm_tail_kernel_rec
#define apm_tail_wide_kernel apm_tail_wide_kernel_rec
#define apm_tail_xwide_kernel apm_tail_xwide_kernel_rec
#define apm_filter_kernel apm_filter_kernel_rec
#define apm_stream_kernel apm_stream_kernel_rec
#define apm_sieve2_kernel apm_sieve2_kernel_rec
#define apm_sieve2cf_kernel apm_sieve2cf_kernel_rec
#define apm_sieve2cfdp_kernel apm_sieve2cfdp_kernel_rec
#define apm_sieve2cfdg_kernel apm_sieve2cfdg_kernel_rec
#define apm_sieve8_kernel apm_sieve8_kernel_rec
#define apm_verify_kernel apm_verify_kernel_rec
#define apm_fused_kernel apm_fused_kernel_rec
/* launchers and their helpers */
#define apm_launch_bitpar apm_launch_bitpar_rec
#define apm_launch_bitpar_wide apm_launch_bitpar_wide_rec
#define apm_launch_bitpar_xwide apm_launch_bitpar_xwide_rec
#define apm_launch_bitlong apm_launch_bitlong_rec
#define apm_launch_wavefront apm_launch_wavefront_rec
#define apm_launch_generic apm_launch_generic_rec
#define apm_launch_nfa apm_launch_nfa_rec
#define apm_launch_tail apm_launch_tail_rec
#define apm_launch_tail_wide apm_launch_tail_wide_rec
#define apm_launch_tail_xwide apm_launch_tail_xwide_rec
#define apm_launch_filter apm_launch_filter_rec
#define apm_launch_stream apm_launch_stream_rec
#define apm_launch_sieve2 apm_launch_sieve2_rec
#define apm_launch_verify apm_launch_verify_rec
#define apm_launch_fused apm_launch_fused_rec
#define apm_bitpar_lds_bytes apm_bitpar_lds_bytes_rec
#define apm_bitlong_lds_bytes apm_bitlong_lds_bytes_rec
#define apm_wavefront_lds_bytes apm_wavefront_lds_bytes_rec
#define apm_nfa_lds_bytes apm_nfa_lds_bytes_rec
#define apm_filter_lds_bytes apm_filter_lds_bytes_rec
#define apm_filter_blocks_per_cu apm_filter_blocks_per_cu_rec
#define apm_filter_fn_b0 apm_filter_fn_b0_rec
#define apm_filter_fn_b1 apm_filter_fn_b1_rec
#define apm_filter_fn_b2 apm_filter_fn_b2_rec
#define apm_filter_fn_b2_dma apm_filter_fn_b2_dma_rec
#define apm_filter_fn_b3 apm_filter_fn_b3_rec
#define apm_stream_blocks_per_cu apm_stream_blocks_per_cu_rec
#define apm_sieve2cf_geometry apm_sieve2cf_geometry_rec
#define apm_sieve2cfdg_fn apm_sieve2cfdg_fn_rec
#define apm_sieve2cf_blocks apm_sieve2cf_blocks_rec
#define apm_verify_geometry apm_verify_geometry_rec
#define apm_fused_lds_bytes apm_fused_lds_bytes_rec
#define apm_fused_geometry apm_fused_geometry_rec
#endif
#endif
