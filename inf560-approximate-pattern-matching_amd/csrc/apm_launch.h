/*
 * apm_launch.h -- host-side launch helpers of the kernel units that size their workgroups at run time (apm_sieve.hip,
 * apm_verify.hip).  They call HIP: included by .hip units only.
 */
#ifndef APM_LAUNCH_H
#define APM_LAUNCH_H

#include <climits>
#include <mutex>
#include <utility>
#include <vector>
#include <hip/hip_runtime.h>

// Raise a kernel's dynamic-LDS limit to the whole CU ONCE per (kernel, device): hipFuncSetAttribute is a host call of tens of
// microseconds, and in front of every launch it showed as kernel time on small inputs (the stream idles while the host works)
static void apm_ensure_max_lds(const void *fn) {
    static std::mutex mu;
    static std::vector<std::pair<const void *, int>> done;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return; }
    std::lock_guard<std::mutex> lock(mu);
    for (const auto &d : done)
        if (d.first == fn && d.second == dev) return;
    (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    done.emplace_back(fn, dev);
}

// The workgroup size that puts the most waves on a CU, and the workgroups per CU it gives (0, *threads = 0: none fits).
// Sizes go from t_first to t_last in steps of t_step (of either sign), and of equal ones the first wins -- from the biggest
// down: the bigger workgroup, fewer copies of the tables.  fn_of(t): the kernel for workgroups of t threads (NULL: none);
// lds_of(t): its dynamic LDS; per_cu_cap: workgroups per CU the caller will use at the most; forced: the only size tried
// (measurement build; 0: all).
template <typename FnOf, typename LdsOf>
static int apm_best_geometry(FnOf &&fn_of, int t_first, int t_last, int t_step, LdsOf &&lds_of, int per_cu_cap, int forced, int *threads) {
    int best_waves = 0, best_blocks = 0;
    *threads = 0;
    for (int t = t_first; t_step > 0 ? t <= t_last : t >= t_last; t += t_step) {
        if (forced && t != forced) continue;
        const void *fn = fn_of(t);
        const size_t lds = lds_of(t);
        if (!fn || lds > (size_t)160 * 1024) continue;
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, t, lds) != hipSuccess || per_cu < 1) {
            (void)hipGetLastError();
            continue;
        }
        per_cu = per_cu > per_cu_cap ? per_cu_cap : per_cu;
        if (per_cu * (t / 64) > best_waves) {
            best_waves = per_cu * (t / 64);
            best_blocks = per_cu;
            *threads = t;
        }
    }
    return best_blocks;
}

#endif /* APM_LAUNCH_H */
