// libd2d_color.so (include/d2d_color.h): conflict-graph RB colouring - DSATUR with a precoloured background - every turn of every
// env in one launch.  gfx950.
//
// Shape: ONE workgroup of 256 threads per env, as d2d_brdyn.hip has it: the colouring couples exactly the links of one env, so the
// workgroup stages the env once and then takes the turns in LDS.
//
// Staging.  The env's [N][N] score block is read once, coalesced along j: the four waves hold the biases of a 256-column chunk
// in registers and walk the receiver rows, four independent loads per lane in flight; the comparisons become the row's words by
// __ballot.  That leaves the DIRECTED bits d(i<-j) in LDS - the diagonal and the columns at or past N never set a bit.  The
// transpose is OR-ed in place with atomicOr: a word read while bits arrive can only carry bits that are in the result anyway, and
// OR does not depend on order.  Per link, by link index: colour (the background's rb, -1 for a link that takes a turn), sat (-1:
// takes no turn or is coloured), deg (the popcount of the row); the loads of the background by atomicAdd; forb and sat of every
// link that takes a turn from its row's coloured neighbours - each thread writes rows it owns only.
//
// A turn: THREADS OWN LINKS (u = tid, tid + 256, ...).  (1) Every uncoloured link's (sat + 1, deg, ~u) as one 64-bit key, reduced
// to the largest - barrier.  (2) Lanes own RBs: nconf[r] is 0 exactly on the RBs outside forb[v], so while an allowed RB is free
// the smallest (pack ? 0 : load, r) over the free ones is the answer, and no tally is taken - barrier.  (3) Only when no allowed RB
// is free: the owners of the chosen row's coloured neighbours tally them by RB (atomicAdd on integers) - barrier - and (nconf,
// pack ? 0 : load, r) of the allowed RBs is reduced to the smallest - barrier.  (4) Every thread holds the same v and r*: the owner
// of v colours it, the owners of its uncoloured neighbours put r* into forb and count it once, the lanes clear a tally that was
// taken.  Two barriers per turn, four on a forced one; what (4) writes is next read by the thread that wrote it or behind the next
// turn's barriers.  No global access inside the turn loop, no global atomics, no floating-point atomics, no
// scratch, nothing that depends on scheduling: the tally and the loads are sums of ones.
#include <hip/hip_runtime.h>

#include <string>

#include "d2d_addon.h"
#include "d2d_color.h"
#include "d2d_wave_key.h"

namespace {

constexpr int CL_THREADS = 256;
constexpr int CL_WAVES = CL_THREADS / 64;
constexpr int CL_CHUNK = 4;                       // 64-column groups a wave has in flight per row

struct ColorArgs {
    const float* score;             // [B][N][N]
    const float* bias;              // [B][N] or null
    const float* thr;               // [B][N]
    const int* rb;                  // [B][N]
    const unsigned* allowed;        // [N][words] or null
    const unsigned char* movable;   // [N] or null
    int* rb_out;
    int* conflicts;
    int* rbs_used;
    unsigned char* proper;
    int N, R;
    int W;                          // ceil(N / 32)
    int words;                      // ceil(R / 32)
    int pack;
    // byte offsets of the LDS arrays behind the adjacency
    unsigned off_forb, off_al, off_col, off_sat, off_deg, off_cnt, off_load, off_used, off_key;
};

// dynamic LDS: adj u32[N][W] | forb u32[N][words] | allowed u32[N][words] (with a mask) | col i32[N] | sat i32[N] | deg i32[N] |
// cnt i32[R] | load i32[R] | used u32[words] | keys u64[2][4]

struct Lds {
    unsigned* adj; unsigned* forb; unsigned* al; int* col; int* sat; int* deg; int* cnt; int* load; unsigned* used;
    unsigned long long* key;
};

__device__ __forceinline__ Lds carve_lds(unsigned char* smem, const ColorArgs& a) {
    Lds s;
    s.adj = reinterpret_cast<unsigned*>(smem);
    s.forb = reinterpret_cast<unsigned*>(smem + a.off_forb);
    s.al = reinterpret_cast<unsigned*>(smem + a.off_al);
    s.col = reinterpret_cast<int*>(smem + a.off_col);
    s.sat = reinterpret_cast<int*>(smem + a.off_sat);
    s.deg = reinterpret_cast<int*>(smem + a.off_deg);
    s.cnt = reinterpret_cast<int*>(smem + a.off_cnt);
    s.load = reinterpret_cast<int*>(smem + a.off_load);
    s.used = reinterpret_cast<unsigned*>(smem + a.off_used);
    s.key = reinterpret_cast<unsigned long long*>(smem + a.off_key);
    return s;
}

using d2d::wave_reduce;                           // the 64-bit key reduction by DPP (d2d_wave_key.h)

// the smallest key of the workgroup, to every thread: one barrier; the four words are next written behind another one
__device__ __forceinline__ unsigned long long block_min(const Lds& s, unsigned long long k, int lane, int wave) {
    k = wave_reduce<false>(k);
    if (lane == 0) s.key[CL_WAVES + wave] = k;
    __syncthreads();
    unsigned long long low = s.key[CL_WAVES];
#pragma unroll
    for (int w = 1; w < CL_WAVES; ++w) {
        const unsigned long long o = s.key[CL_WAVES + w];
        low = o < low ? o : low;
    }
    return low;
}

__global__ __launch_bounds__(CL_THREADS) void color_kernel(const ColorArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const size_t b = blockIdx.x;
    const int N = a.N, R = a.R, W = a.W, words = a.words;
    constexpr int T = CL_THREADS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Lds s = carve_lds(smem, a);
    const float* score = a.score + b * (size_t)N * (size_t)N;
    const float* bias = a.bias ? a.bias + b * (size_t)N : nullptr;
    const float* thr = a.thr + b * (size_t)N;
    const int* rb_row = a.rb + b * (size_t)N;

    // ---- empty tallies, loads and forb rows; the allowed words; the directed bits d(i<-j), every word of every row written once
    for (int k = tid; k < R; k += T) { s.cnt[k] = 0; s.load[k] = 0; }
    for (int k = tid; k < words; k += T) s.used[k] = 0u;
    for (int k = tid; k < N * words; k += T) s.forb[k] = 0u;
    if (a.allowed)
        for (int k = tid; k < N * words; k += T) s.al[k] = a.allowed[k];
    for (int c0 = 0; c0 < N; c0 += 64 * CL_CHUNK) {
        float bj[CL_CHUNK];
#pragma unroll
        for (int k = 0; k < CL_CHUNK; ++k) {
            const int j = c0 + 64 * k + lane;
            bj[k] = bias && j < N ? bias[j] : 0.0f;
        }
        for (int i = wave; i < N; i += CL_WAVES) {
            const float* row = score + (size_t)i * (size_t)N;
            const float t = thr[i];
            float v[CL_CHUNK];
#pragma unroll
            for (int k = 0; k < CL_CHUNK; ++k) {
                const int j = c0 + 64 * k + lane;
                v[k] = j < N ? row[j] : 0.0f;
            }
#pragma unroll
            for (int k = 0; k < CL_CHUNK; ++k) {
                const int j = c0 + 64 * k + lane;
                const float x = bias ? v[k] + bj[k] : v[k];              // one float32 addition, or none
                const unsigned long long m = __ballot(j < N && j != i && x >= t);      // NaN on either side: false
                const int w = (c0 >> 5) + 2 * k;
                if (lane == 0) {
                    if (w < W) s.adj[i * W + w] = (unsigned)m;
                    if (w + 1 < W) s.adj[i * W + w + 1] = (unsigned)(m >> 32);
                }
            }
        }
    }
    __syncthreads();

    // ---- the undirected graph: the transpose OR-ed in place; by link: colour, who takes a turn, the background's loads
    for (int k = tid; k < N * W; k += T) {
        unsigned m = s.adj[k];
        const int i = k / W, w = k - i * W;
        const unsigned bit = 1u << (i & 31);
        while (m) {
            const int j = (w << 5) + __builtin_ctz(m);
            m &= m - 1u;
            atomicOr(&s.adj[j * W + (i >> 5)], bit);
        }
    }
    for (int u = tid; u < N; u += T) {
        bool turn = !a.movable || a.movable[u] != 0;
        if (turn && a.allowed) {
            turn = false;
            for (int w = 0; w < words; ++w) {
                unsigned m = s.al[u * words + w];
                if (w == words - 1 && (R & 31)) m &= (1u << (R & 31)) - 1u;
                if (m) { turn = true; break; }
            }
        }
        const int r = rb_row[u];
        s.col[u] = turn ? -1 : r;
        s.sat[u] = turn ? 0 : -1;
        if (!turn && (unsigned)r < (unsigned)R) atomicAdd(&s.load[r], 1);
    }
    __syncthreads();

    // ---- deg of every link; forb and sat of the links that take a turn, from the coloured neighbours of their rows
    for (int u = tid; u < N; u += T) {
        const bool turn = s.sat[u] >= 0;
        int deg = 0, sat = 0;
        for (int w = 0; w < W; ++w) {
            unsigned m = s.adj[u * W + w];
            deg += __builtin_popcount(m);
            while (turn && m) {
                const int j = (w << 5) + __builtin_ctz(m);
                m &= m - 1u;
                const int c = s.col[j];
                if ((unsigned)c < (unsigned)R) {
                    const unsigned bit = 1u << (c & 31);
                    const unsigned f = s.forb[u * words + (c >> 5)];
                    if (!(f & bit)) { s.forb[u * words + (c >> 5)] = f | bit; ++sat; }
                }
            }
        }
        s.deg[u] = deg;
        if (turn) s.sat[u] = sat;
    }

    // ---- the turns: at most N of them, one link coloured by each
    int conflicts = 0, rbs_used = 0;
    for (int turn = 0; turn < N; ++turn) {
        // (1) the uncoloured link of the largest (sat, deg), ties to the lowest index; key 0: nobody is left
        unsigned long long key = 0ull;
        for (int u = tid; u < N; u += T) {
            const int sat = s.sat[u];
            if (sat < 0) continue;
            const unsigned long long k = ((unsigned long long)(unsigned)(sat + 1) << 32) | ((unsigned long long)(unsigned)s.deg[u] << 16)
                                         | (unsigned long long)(0xFFFFu - (unsigned)u);
            key = k > key ? k : key;
        }
        key = wave_reduce<true>(key);
        if (lane == 0) s.key[wave] = key;
        __syncthreads();
        unsigned long long top = s.key[0];
#pragma unroll
        for (int w = 1; w < CL_WAVES; ++w) {
            const unsigned long long k = s.key[w];
            top = k > top ? k : top;
        }
        if (top == 0ull) break;                                          // every thread read the same words
        const int v = __builtin_amdgcn_readfirstlane((int)(0xFFFFu - ((unsigned)top & 0xFFFFu)));
        // (2) a free RB: the allowed r outside forb[v] of the smallest (pack ? 0 : load, r) - nconf is 0 there and nowhere else
        unsigned long long best = ~0ull;
        for (int r = tid; r < R; r += T) {
            if (a.allowed && !((s.al[v * words + (r >> 5)] >> (r & 31)) & 1u)) continue;
            if ((s.forb[v * words + (r >> 5)] >> (r & 31)) & 1u) continue;
            const unsigned load = a.pack ? 0u : (unsigned)s.load[r];
            const unsigned long long k = ((unsigned long long)load << 16) | (unsigned long long)(unsigned)r;
            best = k < best ? k : best;
        }
        unsigned long long low = block_min(s, best, lane, wave);
        const bool forced = low == ~0ull;                                // every thread read the same words
        if (forced) {
            // (3) no free RB: nconf by RB, tallied by the owners of v's coloured neighbours, then the smallest (nconf, load, r)
            for (int j = tid; j < N; j += T) {
                if (!((s.adj[v * W + (j >> 5)] >> (j & 31)) & 1u)) continue;
                const int c = s.col[j];
                if ((unsigned)c < (unsigned)R) atomicAdd(&s.cnt[c], 1);
            }
            __syncthreads();
            best = ~0ull;
            for (int r = tid; r < R; r += T) {
                if (a.allowed && !((s.al[v * words + (r >> 5)] >> (r & 31)) & 1u)) continue;
                const unsigned load = a.pack ? 0u : (unsigned)s.load[r];
                const unsigned long long k = ((unsigned long long)(unsigned)s.cnt[r] << 32) | ((unsigned long long)load << 16) | (unsigned long long)(unsigned)r;
                best = k < best ? k : best;
            }
            low = block_min(s, best, lane, wave);
            if (low == ~0ull) break;                                     // a link that takes a turn has an allowed RB: not reached
        }
        const int to = __builtin_amdgcn_readfirstlane((int)((unsigned)low & 0xFFFFu));
        const int nconf = __builtin_amdgcn_readfirstlane((int)(unsigned)(low >> 32));
        // (4) colour v; r* joins forb of its uncoloured neighbours; a tally that was taken is cleared for the next one
        const unsigned to_bit = 1u << (to & 31);
        for (int u = tid; u < N; u += T) {
            if (u == v) { s.col[u] = to; s.sat[u] = -1; continue; }
            const int sat = s.sat[u];
            if (sat < 0 || !((s.adj[v * W + (u >> 5)] >> (u & 31)) & 1u)) continue;
            const unsigned f = s.forb[u * words + (to >> 5)];
            if (!(f & to_bit)) { s.forb[u * words + (to >> 5)] = f | to_bit; s.sat[u] = sat + 1; }
        }
        if (forced)
            for (int r = tid; r < R; r += T) s.cnt[r] = 0;
        if (tid == 0) {
            s.load[to] += 1;
            const unsigned seen = s.used[to >> 5];
            if (!(seen & to_bit)) { s.used[to >> 5] = seen | to_bit; ++rbs_used; }
            conflicts += nconf;                                          // every such edge is counted by its later end
        }
    }

    // ---- the results: every colour was last written by the thread that owns the link
    const size_t out_row = b * (size_t)N;
    for (int i = tid; i < N; i += T) a.rb_out[out_row + (size_t)i] = s.col[i];
    if (tid == 0) {
        a.conflicts[b] = conflicts;
        a.rbs_used[b] = rbs_used;
        a.proper[b] = conflicts == 0 ? 1 : 0;
    }
}

unsigned long long round16(unsigned long long x) { return (x + 15ull) & ~15ull; }

}  // namespace

extern "C" int d2d_color_graph(const float* score, const float* tx_bias, const float* rx_thr, const int32_t* rb, int64_t n_envs,
                               int32_t n_links, int32_t n_rbs, const uint32_t* allowed, const uint8_t* movable, int32_t pack,
                               int32_t* rb_out, int32_t* conflicts, int32_t* rbs_used, uint8_t* proper, void* hip_stream) try {
    if (const char* why = check_sizes(n_envs, n_links, D2D_COLOR_MAX_LINKS, n_rbs, D2D_COLOR_MAX_RBS, 1)) return fail(why);
    if (!score || !rx_thr || !rb || !rb_out || !conflicts || !rbs_used || !proper) return fail("null device pointer");
    const void* outs[4] = {rb_out, conflicts, rbs_used, proper};
    for (int x = 0; x < 4; ++x)
        for (int y = x + 1; y < 4; ++y)
            if (outs[x] == outs[y]) return fail("rb_out, conflicts, rbs_used and proper must be four arrays");
    ColorArgs a;
    a.score = score; a.bias = tx_bias; a.thr = rx_thr; a.rb = rb; a.allowed = allowed; a.movable = movable;
    a.rb_out = rb_out; a.conflicts = conflicts; a.rbs_used = rbs_used; a.proper = proper;
    a.N = n_links; a.R = n_rbs; a.pack = pack != 0 ? 1 : 0;
    a.W = (n_links + 31) / 32;
    a.words = (n_rbs + 31) / 32;
    const unsigned long long N = (unsigned long long)n_links, R = (unsigned long long)n_rbs, W = (unsigned long long)a.W,
                             words = (unsigned long long)a.words;
    // 64-bit until the limit is checked: 2048 links x 64 words are 512 KiB of adjacency alone
    unsigned long long off = round16(4ull * N * W);
    a.off_forb = (unsigned)off; off += round16(4ull * N * words);
    a.off_al = (unsigned)off; off += allowed ? round16(4ull * N * words) : 0ull;
    a.off_col = (unsigned)off; off += round16(4ull * N);
    a.off_sat = (unsigned)off; off += round16(4ull * N);
    a.off_deg = (unsigned)off; off += round16(4ull * N);
    a.off_cnt = (unsigned)off; off += round16(4ull * R);
    a.off_load = (unsigned)off; off += round16(4ull * R);
    a.off_used = (unsigned)off; off += round16(4ull * words);
    a.off_key = (unsigned)off; off += 2ull * CL_WAVES * 8ull;
    if (off > (unsigned long long)D2D_COLOR_MAX_LDS_BYTES)
        return fail("n_links and n_rbs need " + std::to_string(off) + " bytes of LDS, more than the " +
                    std::to_string(D2D_COLOR_MAX_LDS_BYTES) + " (D2D_COLOR_MAX_LDS_BYTES) a workgroup can have");
    if (n_envs == 0) return 0;
    const hipError_t e = launch(&color_kernel, dim3((unsigned)n_envs), dim3(CL_THREADS), (unsigned)off,
                                static_cast<hipStream_t>(hip_stream), a);
    if (e != hipSuccess) return fail(std::string("color_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

D2D_ADDON_LAST_ERROR(d2d_color_last_error)
