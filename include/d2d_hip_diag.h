/*
 * d2d_hip_diag.h - measurement equipment around libd2d_hip.so.  NOT part of the drop-in boundary (that is d2d_hip.h, which
 * INTEGRATION.md binds): nothing here replaces an interface of the reference.  Three things live here:
 *
 *  (1) tuning keys / values that only a DIAGNOSTIC build of libd2d_hip.so accepts
 *      (D2D_BUILD_DIAG=1 python -m gym_d2d_amd.build; a release build answers D2D_ERR_UNSUPPORTED): the A/B shapes the
 *      kernels were tuned against, the ablation switch of the generic step kernel and the phase stamps of tools/phase_times.py;
 *  (2) the write-ceiling probe, a library of its own (libd2d_probe.so, csrc/d2d_probe.hip): what bench.py's
 *      `box_write_ceiling` and the placement studies under profiles/ were measured with;
 *  (3) the same library's second source (csrc/d2d_devfn.hip): the device functions the kernels share, each behind a wrapper
 *      kernel, for tests/test_gpu_devfn.py.
 */
#ifndef D2D_HIP_DIAG_H
#define D2D_HIP_DIAG_H

#include "d2d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- (1) diagnostic builds of libd2d_hip.so: further d2d_set_tuning keys ------------------------------------------------ */
#define D2D_TUNE_OBS_VARIANT 4   /* 0 (default): flat 32 KB slabs, T staged in LDS; 1: T read from global; 3: the row-aligned
                                    kernel of rounds 1-3                                                                    */
#define D2D_TUNE_STEP_ABLATE 9   /* the one key that DOES change results: bit mask of kernel parts to skip (1 interferer walk,
                                    2 mask build, 4 mask clear, 8 result stores, 16 table store, 32 rb/pwr stores, 64 pass-0/1
                                    barriers, 128 per-env loads hit L2, ...) so that the rest can be timed                   */
#define D2D_TUNE_OBS_STAGGER 16  /* wave w of an obs workgroup sleeps w * value * 64 clocks before its stores; 0 = off; the
                                    row-aligned kernel (D2D_TUNE_OBS_VARIANT 3) only: the flat kernels' arguments are the
                                    preloaded scalars and carry no diagnostic word                                        */
/* ... and further VALUES of release keys: D2D_TUNE_OBS_NONTEMPORAL 2 sc1, 3 sc0 sc1, 4 sc0 sc1 nt (the scope bits of the
 * gfx942+ store encoding; 5 sc1 nt is the flat kernels' default and a release value, d2d_hip.h); D2D_TUNE_STEP_WALK 1 =
 * membership masks, flattened walk.                                                                                         */

/* diagnostic builds only: copy the shader-clock stamps of the last step (D2D_TUNE_STEP_ABLATE bit 8192) to the host          */
int d2d_debug_stamps(d2d_handle* h, void* host, size_t bytes);

/* ---- (2) libd2d_probe.so: streaming-store probe ---------------------------------------------------------------------------
 * Writes a scratch buffer of `bytes` (>= 64 MiB; rounded down to whole groups of eight 512-row regions) `iters` times with
 * pure fill kernels - nothing to compute - in a family of store geometries that contains the obs kernel's own, and with
 * hipMemsetAsync, and reports the BEST sustained rate: the box's write ceiling as far as these kernels can demonstrate one.
 * per_variant (n entries, may be NULL) receives the first n rates (variant v: block {768,1024,512,256}[v & 3], rows per
 * workgroup {2,4,8,32}[(v >> 2) & 3], nontemporal unless v & 16; index D2D_PROBE_VARIANTS = hipMemsetAsync).  Runs on the null
 * stream of `device` and synchronises the device around itself.  Returns 0, or 1 with text in d2d_probe_last_error().        */
#define D2D_PROBE_VARIANTS 32
int d2d_probe_write_variants(int32_t device, size_t bytes, int32_t iters, double* best_gb_per_s, double* per_variant, int32_t n);
/* One member of the family with the obs kernel's TIMING structure added: variant = the geometry index above + 32 (every
 * workgroup first stages one row of a table through LDS behind a barrier and stores what it reads back) + 64 (wave w sleeps
 * w * stagger * 64 clocks before its first store) + 128 * k (k = 1 .. 4: the store's cache policy sc1 / sc0 sc1 / sc0 sc1 nt /
 * sc1 nt instead of nt or plain).  dst_dev = NULL writes a scratch buffer of `bytes`; a device pointer writes THAT memory.  */
int d2d_probe_write_staged(int32_t device, void* dst_dev, size_t bytes, int32_t variant, int32_t stagger, int32_t iters,
                           double* gb_per_s);
const char* d2d_probe_last_error(void);

/* ---- (3) libd2d_probe.so: the shared device functions, one at a time (csrc/d2d_devfn.hip) ----------------------------------
 * The functions the kernels share (csrc/d2d_step_device.h, d2d_wave_key.h, d2d_same_rb.h) behind thin wrapper kernels - load
 * the arguments, call the header's function, store what it returns - so that a test can hold each against a float64 or exact
 * integer reference of its own (tests/test_gpu_devfn.py).  Every pointer is device memory; n counts what `fn` states below.
 *                                  a                 b                c            out0               out1         k0, k1
 *   POW10_TENTH                    i32 p[n]                                        f32[n]
 *   POW_NEG_HALF                   f32 d2[n]         f32 head[n]      f32 tail[n]  f32[n]
 *   POW_K_GAINS                    f32 d2[n]         f32 phi[n]                    f32[n]                          k, form
 *     form 0: pow_k_gains<1>, k at run time; 1: pow_k_gains<4>, four consecutive pairs per thread; 2: pow_k_gains<1, 4> (k == 4)
 *   PAIR_GAIN                      f32 d2[n]         f32 head|phi[n]  f32 tail[n]  f32[n]                          mode, k
 *     mode 0: pair_gain<PL_INV_SQUARE>, 1: pair_gain<PL_POWER>, 4: pair_gain<PL_POWK> (the values of PlMode, d2d_internal.h)
 *   PRECISE_DIV, FAST_DIV          f32 x[n]          f32 y[n]                      f32[n]
 *   COS_TURNS                      f32 u[n]                                        f32[n]
 *   PHILOX_STEP                    u32 ctr[n][4]     u32 key[n][2]                 u32 o0[n]          u32 o1[n]
 *   PHILOX_NORMAL                  u32 ctr[n][4]     u32 key[n][2]                 f32 z[n]
 *     ctr = (env, step, ctr2, kind), key = (seed_lo, seed_hi)
 *   WAVE_SUM                       f32[n]                                          f32[n]                          block
 *   WAVE_SUM_HALVES                f32[n]                                          f32 lo[n]          f32 hi[n]    block
 *   WAVE_MAX, WAVE_MIN             u64[n]                                          u64[n]                          block
 *     workgroups of `block` (64 or 256) threads, n a multiple of it: every lane stores the value its wave returned
 *   SORT8                          u32[n][8]                                       u32[n][8]
 *   OBS_SRC_COL                    u32 f[n]          u32 i[n]                      u32[n]
 *   SAME_RB                        i32 rb[n][N]                                    i32 slot[n][N]     i32[n][R+2]  N, R
 *     one workgroup per env, staged in LDS as the kernels stage it (keys, barrier, rank, barrier, starts); out1 is the R + 2 words
 *     of LDS from start[0] on, which the wrapper fills with D2D_DEVFN_SENTINEL before same_rb_starts runs: start[0 .. R], and the
 *     word behind them.
 * Launches on `hip_stream` and does not wait for it.  n == 0 returns 0 without a launch.  Returns 0, or 1 with text in
 * d2d_probe_last_error(): an unknown fn, n < 0, a block, form, mode, k, N or R outside what is stated, a null pointer among the
 * ones `fn` takes - all refused before anything is launched.                                                              */
enum d2d_devfn {
    D2D_DEVFN_POW10_TENTH = 0,
    D2D_DEVFN_POW_NEG_HALF = 1,
    D2D_DEVFN_POW_K_GAINS = 2,
    D2D_DEVFN_PAIR_GAIN = 3,
    D2D_DEVFN_PRECISE_DIV = 4,
    D2D_DEVFN_FAST_DIV = 5,
    D2D_DEVFN_COS_TURNS = 6,
    D2D_DEVFN_PHILOX_STEP = 7,
    D2D_DEVFN_PHILOX_NORMAL = 8,
    D2D_DEVFN_WAVE_SUM = 9,
    D2D_DEVFN_WAVE_SUM_HALVES = 10,
    D2D_DEVFN_WAVE_MAX = 11,
    D2D_DEVFN_WAVE_MIN = 12,
    D2D_DEVFN_SORT8 = 13,
    D2D_DEVFN_OBS_SRC_COL = 14,
    D2D_DEVFN_SAME_RB = 15,
    D2D_DEVFN_COUNT = 16
};
#define D2D_DEVFN_SENTINEL 0x5A5A5A5A
int d2d_probe_device_fn(int32_t fn, const void* a, const void* b, const void* c, void* out0, void* out1, int64_t n, int32_t k0,
                        int32_t k1, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* D2D_HIP_DIAG_H */
