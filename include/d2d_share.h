/* libd2d_share.so - exact optimal RB sharing for small link groups: the value of every subset of the movable links on every RB,
 * and the max-plus subset convolution over the RBs that places them optimally, several links per RB
 * (gym_d2d_amd.envs.VecD2DEnv.sharing_values, solve_sharing, share_rbs, share_rbs_actions).
 *
 * Separate from libd2d_hip.so (include/d2d_hip.h), whose exported set is fixed per ABI version, and stateless: no handle, raw
 * device pointers of this process's current HIP device, asynchronous on hip_stream (NULL: the null stream).
 *
 * The decomposition.  With the background (every link that is not movable) fixed on its RB at its power, links on different RBs
 * do not interfere, so the total capacity of a placement of the n_movable movable links is a sum over the RBs of a term that
 * depends only on WHICH SUBSET S of the movable links sits on that RB.  A subset is a mask: bit a is movable_links[a].
 *
 * d2d_share_values writes that term for every (env, RB, subset):
 *
 *   values[b][r][S]  the sum, in double, in ascending link index, of the float32 capacities of the background members of r and
 *                    the links of S, when exactly those links are on r.  Every capacity is the step's (and d2d_evaluate's) for
 *                    that state, bit for bit: the interference a member receives is summed over the other members in ascending
 *                    link index, float products into a double accumulator, then the step's operations.  values[b][r][0] is the
 *                    background of r alone (0.0 for an RB without one)
 *   allowed          a subset with a link that is not allowed on r is -inf
 *   closed_rb[b][r]  1 iff the background of r has more than D2D_SHARE_MAX_BACKGROUND members: such an RB is CLOSED - every
 *                    S != 0 entry is -inf, the S = 0 entry is still the true capacity of its background - else 0
 *
 *   pos_x, pos_y     f32 [n_envs][n_dev]
 *   rb, pwr_dbm      i32 [n_envs][n_links]: the decoded planes; a background link whose rb is outside [0, n_rbs) is on no RB and
 *                    in no term.  The rb entries of the movable links play no part, their pwr_dbm entries are their powers
 *   link_tx, link_rx i32 [n_links]; dev_cols f32 [6][n_dev], cap_cols f32 [2][n_dev]; law, pow_k: as d2d_evaluate takes them
 *   movable_links    i32 [n_movable] on the device: distinct link indices in ascending order (the caller's promise)
 *   allowed          NULL: every RB, else u32 [n_links][ceil(n_rbs / 32)]: bit r & 31 of word r / 32
 *   values           f64 [n_envs][n_rbs][2^n_movable]
 *   closed_rb        i32 [n_envs][n_rbs]
 *
 * Grid (env, RB), 256 threads.  The workgroup compacts the background members of its RB by wave ballots (no atomics: the same
 * order on every call), merges them with the movable links in ascending link index, stages them as d2d_evaluate stages tuples and
 * computes the float32 term matrix term[j -> i] of all (member or movable)^2 pairs ONCE into LDS - a precomputed term is the same
 * float the on-the-fly product gives.  Threads then own subsets (stride 256) and walk the matrix at wave-uniform addresses.
 * With U = min(n_links, D2D_SHARE_MAX_BACKGROUND) + n_movable, L = n_links + D2D_SHARE_MAX_MOVABLE and round16 rounding up to
 * 16 bytes, a workgroup needs
 *
 *   round16(8 ceil(n_links / 64)) + round16(4 U) + round16(4 U (U | 1)) + 32 L + 2 round16(4 L) + round16(8 L)
 *
 * bytes of LDS, and round16(8 L) more under the power laws, which must fit D2D_SHARE_MAX_LDS_BYTES.
 *
 * d2d_share_solve takes ANY f64 [n_envs][n_rbs][2^n_movable] block and solves, per env,
 *
 *   g_-1[0] = 0, g_-1[T != 0] = -inf
 *   g_r[T]  = max over S subset of T, S admissible on r, of  g_(r-1)[T \ S] + values[b][r][S]         r = 0 .. n_rbs - 1
 *
 *   admissible  S is admissible on r iff values[b][r][S] is finite (NaN, +inf and -inf are never chosen) and
 *               popcount(S) <= quota[r] (quota NULL: no limit; a negative quota is read as 0, which closes r to movable links)
 *   ties        equal sums (a double comparison) go to the numerically lowest S
 *   result      backtracking from T = 2^n_movable - 1 at the last RB gives col[b][a], the RB of mask bit a; value[b] is
 *               g_(n_rbs - 1)[2^n_movable - 1].  An env in which that is -inf is infeasible: every col -1, value 0.0, feasible 0;
 *               it does not disturb the others
 *
 * Every candidate is ONE double addition and max is exact, so the result does not depend on the order of evaluation: two calls
 * give the same words, and a sequential restatement gives them too.
 *
 *   quota        NULL or i32 [n_rbs] on the device, the same for every env
 *   choice       u16 [n_envs][n_rbs][2^n_movable]: the chosen S of every (RB, T), written and read back by the kernel
 *   col          i32 [n_envs][n_movable]; value f64 [n_envs]; feasible i32 [n_envs]
 *
 * One workgroup per env takes every RB in one launch: two layers g of 2^n_movable doubles, the RB's staged values and its choice
 * words live in LDS, 26 * 2^n_movable bytes, which must fit D2D_SHARE_MAX_LDS_BYTES - the reason n_movable stops at
 * D2D_SHARE_MAX_MOVABLE.  A WAVE owns a target T: lane l takes the submasks whose low six bits are l, so the wave reads 64
 * consecutive doubles of each array per step, and a fixed reduction tree picks (largest sum, lowest S).
 *
 * 1 <= n_movable <= D2D_SHARE_MAX_MOVABLE, 1 <= n_links <= D2D_SHARE_MAX_LINKS, 1 <= n_rbs <= D2D_SHARE_MAX_RBS, n_envs >= 0 (0:
 * nothing to do); values and choice together hold at most D2D_SHARE_MAX_BLOCK_BYTES.  No floating-point atomics, no global
 * atomics, no scratch memory.  Both return 0, or non-zero with a message in d2d_share_last_error().                             */
#ifndef D2D_SHARE_H
#define D2D_SHARE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_SHARE_LAW_INV_SQUARE 0
#define D2D_SHARE_LAW_POWER 1
#define D2D_SHARE_LAW_POW_K 2
#define D2D_SHARE_MAX_LINKS 2048
#define D2D_SHARE_MAX_RBS 8192
/* the movable links of one call: two layers of 2^12 doubles and an RB's staged values are 96 KiB of LDS */
#define D2D_SHARE_MAX_MOVABLE 12
/* the background members an RB may have and still take movable links */
#define D2D_SHARE_MAX_BACKGROUND 64
/* the LDS one workgroup can get on gfx950 (160 KiB) */
#define D2D_SHARE_MAX_LDS_BYTES 163840
/* the bytes the value block and the choice words of one call may hold together (8 GiB) */
#define D2D_SHARE_MAX_BLOCK_BYTES 8589934592

int d2d_share_values(const float* pos_x, const float* pos_y, const int32_t* rb, const int32_t* pwr_dbm, const int32_t* link_tx,
                     const int32_t* link_rx, const float* dev_cols, const float* cap_cols, int32_t law, int32_t pow_k,
                     int64_t n_envs, int32_t n_dev, int32_t n_links, int32_t n_rbs, const int32_t* movable_links,
                     int32_t n_movable, const uint32_t* allowed, double* values, int32_t* closed_rb, void* hip_stream);
int d2d_share_solve(const double* values, const int32_t* quota, int64_t n_envs, int32_t n_rbs, int32_t n_movable,
                    uint16_t* choice, int32_t* col, double* value, int32_t* feasible, void* hip_stream);
const char* d2d_share_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* D2D_SHARE_H */
