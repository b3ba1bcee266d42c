// libd2d_stable.so (include/d2d_stable.h): stable RB matching with quotas - deferred acceptance with the links proposing - every
// round of every env in one launch.  gfx950.
//
// Shape: ONE workgroup of 256 threads per env, as d2d_color.hip has it: a matching couples exactly the links and RBs of one env, so
// the workgroup keeps the env's state in LDS and takes the rounds there.  The two preference blocks, 8 M R bytes per env, stay in
// global memory / L2 and are read by rows, lanes across r, with plain 4-byte loads: a row of an odd R is not 16-byte aligned.
//
// Keys.  A float32 becomes an unsigned word of the same order (sign bit flipped, negatives complemented) after -0.0 is made +0.0,
// so that the two zeros tie as the float32 comparison has them.  A link's key of RB r is (ordered link_pref, ~r): larger is
// better, ties to the lower r; an RB's key of link a is (ordered rb_pref, ~a) likewise.  No key of an acceptable pair is 0 or all
// ones (finite values order strictly inside), so a cursor of all ones is "nothing proposed yet" and a best of 0 "nothing left".
//
// A round.  (1) WAVES OWN PROPOSERS: the free links with something left are a list in LDS; wave w takes its entries w, w + 4, ...
// For one link all 64 lanes scan its two rows for the largest key strictly behind its cursor among the acceptable pairs - a 64-bit
// reduction by DPP (d2d_wave_key.h).  Lane 0 moves the cursor there, takes the RB's liking of the link from the lane that read it
// (readlane: no second load), and pushes the link on the RB's list of proposers (atomicExch on the list head).  A link with
// nothing left leaves the lists for good - barrier.  (2) THREADS
// OWN RBs: the thread of an RB that was proposed to walks its proposers.  The holders of an RB are a list in ascending order of the
// RB's keys, so the worst holder is its head: under quota a proposer is inserted; at quota it displaces the head if the RB likes
// it better, else it is rejected; whoever is left out is pushed on the NEXT round's list of free links (atomicAdd on its length) -
// barrier.  The rounds end when that list is empty, read by every thread from one LDS word behind the barrier: no iteration cap.
//
// The order in which proposers reach a list depends on scheduling; the result does not: an RB ends a round with the best quota of
// (holders, proposers) whatever the order, and deferred acceptance reaches the one link-optimal stable matching, making the same
// proposals, in every order (McVitie and Wilson).  Integer LDS atomics only, no global atomics, no floating-point atomics, no
// scratch; inside the rounds global memory is only read.
#include <hip/hip_runtime.h>

#include <string>

#include "d2d_addon.h"
#include "d2d_same_rb.h"
#include "d2d_stable.h"
#include "d2d_wave_key.h"

namespace {

using d2d::wave_reduce;

static_assert(D2D_STABLE_MAX_LINKS == d2d::SAME_RB_MAX_LINKS && D2D_STABLE_MAX_RBS == d2d::SAME_RB_MAX_RBS,
              "the limits of every kernel that keeps an env in LDS");

constexpr int SM_THREADS = 256;
constexpr int SM_WAVES = SM_THREADS / 64;
constexpr int SM_CHUNK = 4;                       // 64-column groups of both rows a wave has in flight

struct StableArgs {
    const float* link_pref;         // [B][M][R]
    const float* rb_pref;           // [B][M][R]
    const int* quota;               // [R]
    int* col;                       // [B][M]
    int* load;                      // [B][R]
    int* proposals;                 // [B]
    int* unmatched;                 // [B]
    int M, R;
    int list_stride;                // the ints between the two lists of free links
    // byte offsets of the LDS arrays behind the cursors
    unsigned off_rk, off_next, off_match, off_list, off_quota, off_load, off_worst, off_prop, off_misc;
};

// dynamic LDS: cursor u64[M] | rk u64[M] | next i32[M] | match i32[M] | free i32[2][M] | quota i32[R] | load i32[R] | worst i32[R] |
// prop i32[R] | misc i32[4]: the lengths of the two free lists, the proposals, the unmatched
struct Lds {
    unsigned long long* cursor; unsigned long long* rk; int* next; int* match; int* free; int* quota; int* load; int* worst; int* prop;
    int* misc;
};

__device__ __forceinline__ Lds carve_lds(unsigned char* smem, const StableArgs& a) {
    Lds s;
    s.cursor = reinterpret_cast<unsigned long long*>(smem);
    s.rk = reinterpret_cast<unsigned long long*>(smem + a.off_rk);
    s.next = reinterpret_cast<int*>(smem + a.off_next);
    s.match = reinterpret_cast<int*>(smem + a.off_match);
    s.free = reinterpret_cast<int*>(smem + a.off_list);
    s.quota = reinterpret_cast<int*>(smem + a.off_quota);
    s.load = reinterpret_cast<int*>(smem + a.off_load);
    s.worst = reinterpret_cast<int*>(smem + a.off_worst);
    s.prop = reinterpret_cast<int*>(smem + a.off_prop);
    s.misc = reinterpret_cast<int*>(smem + a.off_misc);
    return s;
}

// the unsigned word whose order is the float32 order of x, the two zeros being one value
__device__ __forceinline__ unsigned ordered(float x) {
    const unsigned u = x == 0.0f ? 0u : __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ bool finite(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

__device__ __forceinline__ unsigned long long key_of(float x, int index) {
    return ((unsigned long long)ordered(x) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)index);
}

__global__ __launch_bounds__(SM_THREADS) void stable_kernel(const StableArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const size_t b = blockIdx.x;
    const int M = a.M, R = a.R;
    constexpr int T = SM_THREADS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Lds s = carve_lds(smem, a);
    const float* link_pref = a.link_pref + b * (size_t)M * (size_t)R;
    const float* rb_pref = a.rb_pref + b * (size_t)M * (size_t)R;

    // ---- every link free with nothing proposed, every RB empty; the first list of free links is every link
    for (int l = tid; l < M; l += T) { s.cursor[l] = ~0ull; s.match[l] = -1; s.free[l] = l; }
    for (int r = tid; r < R; r += T) {
        const int q = a.quota[r];
        s.quota[r] = q > 0 ? q : 0;
        s.load[r] = 0; s.worst[r] = -1; s.prop[r] = -1;
    }
    if (tid == 0) { s.misc[0] = M; s.misc[1] = 0; s.misc[2] = 0; s.misc[3] = 0; }
    __syncthreads();

    // ---- the rounds: list p holds this round's free links, list p ^ 1 collects the next round's
    int made = 0;                                                        // the proposals lane 0 of this wave has made
    for (int p = 0;; p ^= 1) {
        const int n = s.misc[p];                                         // every thread reads the same word, behind a barrier
        if (n == 0) break;
        const int* now = s.free + p * a.list_stride;
        int* then = s.free + (p ^ 1) * a.list_stride;
        // (1) every free link proposes to the best acceptable RB strictly behind its cursor, or leaves
        for (int i = wave; i < n; i += SM_WAVES) {
            const int l = __builtin_amdgcn_readfirstlane(now[i]);
            const unsigned long long cursor = s.cursor[l];
            const float* x = link_pref + (size_t)l * (size_t)R;
            const float* y = rb_pref + (size_t)l * (size_t)R;
            unsigned long long best = 0ull;
            float liking = 0.0f;                                         // rb_pref at this lane's best: the RB's liking of the link
            for (int c0 = 0; c0 < R; c0 += 64 * SM_CHUNK) {
                float v[SM_CHUNK], w[SM_CHUNK];
#pragma unroll
                for (int k = 0; k < SM_CHUNK; ++k) {
                    const int r = c0 + 64 * k + lane;
                    v[k] = r < R ? x[r] : __builtin_inff();             // past the row: unacceptable
                    w[k] = r < R ? y[r] : __builtin_inff();
                }
#pragma unroll
                for (int k = 0; k < SM_CHUNK; ++k) {
                    const unsigned long long key = key_of(v[k], c0 + 64 * k + lane);
                    if (finite(v[k]) && finite(w[k]) && key < cursor && key > best) { best = key; liking = w[k]; }
                }
            }
            const unsigned long long top = wave_reduce<true>(best);
            if (top != 0ull) {                                           // the same scalar in every lane
                // keys are distinct, so exactly one lane holds the wave's: its liking comes by readlane, not by another load
                const int holder = __builtin_ctzll(__ballot(best == top));
                const float liked = __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(liking), holder));
                if (lane == 0) {
                    const int r = (int)(0xFFFFFFFFu - (unsigned)top);
                    s.cursor[l] = top;
                    s.rk[l] = key_of(liked, l);
                    s.next[l] = atomicExch(&s.prop[r], l);
                    ++made;
                }
            }
        }
        __syncthreads();
        if (tid == 0) s.misc[p] = 0;                                     // read by everyone before the barrier; filled again next round
        // (2) every RB that was proposed to keeps the best quota[r] of (holders, proposers); who is left out is free next round
        for (int r = tid; r < R; r += T) {
            int c = s.prop[r];
            if (c < 0) continue;
            s.prop[r] = -1;
            const int q = s.quota[r];
            int load = s.load[r], head = s.worst[r];
            while (c >= 0) {
                const int after = s.next[c];
                const unsigned long long k = s.rk[c];
                int out = c;                                             // who this proposer leaves out: itself, the worst holder, nobody
                if (load < q) {
                    ++load; out = -1;
                } else if (q > 0 && k > s.rk[head]) {
                    out = head; head = s.next[head];
                    s.match[out] = -1;
                }
                if (out != c) {                                          // c is held: into the ascending list, the worst at the head
                    if (head < 0 || k < s.rk[head]) {
                        s.next[c] = head; head = c;
                    } else {
                        int at = head;
                        for (int nx = s.next[at]; nx >= 0 && s.rk[nx] < k; nx = s.next[at]) at = nx;
                        s.next[c] = s.next[at]; s.next[at] = c;
                    }
                    s.match[c] = r;
                }
                if (out >= 0) then[atomicAdd(&s.misc[p ^ 1], 1)] = out;      // at most one per proposer: never past M
                c = after;
            }
            s.load[r] = load; s.worst[r] = head;
        }
        __syncthreads();
    }

    // ---- the results: every match and load was last written behind the last barrier
    int un = 0;
    for (int l = tid; l < M; l += T) {
        const int m = s.match[l];
        a.col[b * (size_t)M + (size_t)l] = m;
        un += m < 0 ? 1 : 0;
    }
    for (int r = tid; r < R; r += T) a.load[b * (size_t)R + (size_t)r] = s.load[r];
    if (lane == 0 && made) atomicAdd(&s.misc[2], made);
    if (un) atomicAdd(&s.misc[3], un);
    __syncthreads();
    if (tid == 0) { a.proposals[b] = s.misc[2]; a.unmatched[b] = s.misc[3]; }
}

unsigned long long round16(unsigned long long x) { return (x + 15ull) & ~15ull; }

}  // namespace

extern "C" int d2d_stable_match(const float* link_pref, const float* rb_pref, const int32_t* quota, int64_t n_envs, int32_t n_links,
                                int32_t n_rbs, int32_t* col, int32_t* load, int32_t* proposals, int32_t* unmatched,
                                void* hip_stream) try {
    if (const char* why = check_sizes(n_envs, n_links, D2D_STABLE_MAX_LINKS, n_rbs, D2D_STABLE_MAX_RBS, 1)) return fail(why);
    if (!link_pref || !rb_pref || !quota || !col || !load || !proposals || !unmatched) return fail("null device pointer");
    const void* outs[4] = {col, load, proposals, unmatched};
    for (int x = 0; x < 4; ++x)
        for (int y = x + 1; y < 4; ++y)
            if (outs[x] == outs[y]) return fail("col, load, proposals and unmatched must be four arrays");
    StableArgs a;
    a.link_pref = link_pref; a.rb_pref = rb_pref; a.quota = quota;
    a.col = col; a.load = load; a.proposals = proposals; a.unmatched = unmatched;
    a.M = n_links; a.R = n_rbs;
    const unsigned long long M = (unsigned long long)n_links, R = (unsigned long long)n_rbs;
    unsigned long long off = round16(8ull * M);
    a.off_rk = (unsigned)off; off += round16(8ull * M);
    a.off_next = (unsigned)off; off += round16(4ull * M);
    a.off_match = (unsigned)off; off += round16(4ull * M);
    a.off_list = (unsigned)off; a.list_stride = (int)(round16(4ull * M) / 4ull); off += 2ull * round16(4ull * M);
    a.off_quota = (unsigned)off; off += round16(4ull * R);
    a.off_load = (unsigned)off; off += round16(4ull * R);
    a.off_worst = (unsigned)off; off += round16(4ull * R);
    a.off_prop = (unsigned)off; off += round16(4ull * R);
    a.off_misc = (unsigned)off; off += 16ull;
    if (off > (unsigned long long)D2D_STABLE_MAX_LDS_BYTES)
        return fail("n_links and n_rbs need " + std::to_string(off) + " bytes of LDS, more than the " +
                    std::to_string(D2D_STABLE_MAX_LDS_BYTES) + " (D2D_STABLE_MAX_LDS_BYTES) a workgroup can have");
    if (n_envs == 0) return 0;
    const hipError_t e = launch(&stable_kernel, dim3((unsigned)n_envs), dim3(SM_THREADS), (unsigned)off,
                                static_cast<hipStream_t>(hip_stream), a);
    if (e != hipSuccess) return fail(std::string("stable_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

D2D_ADDON_LAST_ERROR(d2d_stable_last_error)
