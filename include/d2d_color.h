/* libd2d_color.so - conflict-graph RB colouring, DSATUR with precolouring (gym_d2d_amd.envs.VecD2DEnv.color_graph, color_rbs,
 * color_rbs_actions).
 *
 * Separate from libd2d_hip.so (include/d2d_hip.h), whose exported set is fixed per ABI version, and stateless: no handle, raw
 * device pointers of this process's current HIP device, asynchronous on hip_stream (NULL: the null stream).
 *
 * d2d_color_graph colours, per env b, the links that take a turn with the RBs 0 .. n_rbs - 1:
 *
 *   conflict   d(i<-j) = (i != j) and (score[b][i][j] + tx_bias[b][j] >= rx_thr[b][i])     one float32 addition (none with
 *              tx_bias NULL), one float32 comparison: a NaN on either side compares false, rx_thr = +inf makes link i never a
 *              victim, rx_thr = -inf makes every entry that is not NaN conflict
 *   edge       {i, j} iff d(i<-j) or d(j<-i);  deg[i] = the number of i's neighbours, whatever they are
 *   turn       link i takes a turn iff movable[i] != 0 and it has an allowed RB in [0, n_rbs).  Every other link is background: it
 *              keeps rb[b][i] and is coloured from the start; a background rb outside [0, n_rbs) is on no RB - it colours
 *              nothing and is counted nowhere.  A link that takes a turn starts uncoloured, its current RB is not read
 *   forb[v]    the RBs in [0, n_rbs) held by coloured neighbours of v;  sat[v] = their number, allowed for v or not
 *   load[r]    the coloured links on r, background included
 *   until every link that takes a turn is coloured:
 *     v        = the uncoloured one of the largest (sat, deg), ties to the lowest link index
 *     nconf[r] = the coloured neighbours of v on r, for every r allowed to v
 *     r*       = the allowed r of the smallest (nconf[r], pack ? 0 : load[r], r), compared lexicographically
 *     colour v with r*: load[r*] += 1, and r* joins forb[u] of every uncoloured neighbour u
 *
 * pack = 0 spreads: a free RB with the fewest links on it.  pack != 0 is the classic greedy: the lowest free RB.  With no free RB
 * either rule degrades to the least-conflicting one.  A heuristic: no optimality is claimed for the colours used or the conflicts
 * left.  Integers only behind the comparison, LDS atomics on integers only, no global atomics: two calls give the same words.
 *
 *   score        f32 [n_envs][n_links][n_links], receiver-major: i receives, j transmits (d2d_graph_coupling's layout)
 *   tx_bias      f32 [n_envs][n_links] or NULL: added to column j.  NULL: 0, nothing is added
 *   rx_thr       f32 [n_envs][n_links]: the threshold of row i
 *   rb           i32 [n_envs][n_links]: the current RBs; read for the background only
 *   n_envs, n_links, n_rbs
 *   allowed      u32 [n_links][ceil(n_rbs / 32)] or NULL: bit r & 31 of word r / 32 of row i - link i may take RB r
 *                (gym_d2d_amd.best_response.pack_allowed).  NULL: every RB
 *   movable      u8 [n_links] or NULL: 0 - the link is background.  NULL: every link is movable
 *   pack         0: spread over the RBs; otherwise: pack into the lowest
 *   rb_out       i32 [n_envs][n_links]: the colours; background rows are copied through, whatever they hold
 *   conflicts    i32 [n_envs]: the edges {i, j} with an end that took a turn whose two ends are on the same RB in [0, n_rbs)
 *   rbs_used     i32 [n_envs]: the distinct RBs the links that took a turn hold
 *   proper       u8 [n_envs]: conflicts == 0
 *
 * One workgroup of 256 threads per env keeps the env in LDS across all turns: the adjacency bitset, forb, the allowed words,
 * colour / sat / deg by link, the tally and the loads by RB.  With W = ceil(n_links / 32), words = ceil(n_rbs / 32) and round16
 * rounding up to 16 bytes, a workgroup needs
 *
 *   round16(4 n_links W) + (1 + has_allowed) round16(4 n_links words) + 3 round16(4 n_links) + 2 round16(4 n_rbs)
 *     + round16(4 words) + 64
 *
 * bytes, which must fit D2D_COLOR_MAX_LDS_BYTES.  1 <= n_links <= D2D_COLOR_MAX_LINKS, 1 <= n_rbs <= D2D_COLOR_MAX_RBS,
 * n_envs >= 0 (0: nothing to do); no link taking a turn is legal (the background is scored: conflicts 0, rbs_used 0, proper 1).
 * No scratch memory; at most 64 VGPRs.  The four outputs must be four arrays.  Returns 0, or non-zero with a message in
 * d2d_color_last_error().                                                                                                       */
#ifndef D2D_COLOR_H
#define D2D_COLOR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_COLOR_MAX_LINKS 2048
#define D2D_COLOR_MAX_RBS 8192
/* the LDS one workgroup can get on gfx950 (160 KiB) */
#define D2D_COLOR_MAX_LDS_BYTES 163840

int d2d_color_graph(const float* score, const float* tx_bias, const float* rx_thr, const int32_t* rb, int64_t n_envs,
                    int32_t n_links, int32_t n_rbs, const uint32_t* allowed, const uint8_t* movable, int32_t pack,
                    int32_t* rb_out, int32_t* conflicts, int32_t* rbs_used, uint8_t* proper, void* hip_stream);
const char* d2d_color_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* D2D_COLOR_H */
