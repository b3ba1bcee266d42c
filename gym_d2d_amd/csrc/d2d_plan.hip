// Launch planner of the step: the one statement of which kernel serves a step and in what shape (see d2d_plan.h).  Host code
// only; every number below was measured on an MI355X (the evidence lies under profiles/, named where it is used).
#include "../../include/d2d_hip.h"
#include "d2d_plan.h"

#include <cstring>

namespace d2d {

namespace {

StepLds step_lds_layout(int N, int R, int mask_words, int fuse_obs, int lpt, int reward_fn, int mode, int lists, int xpos) {
    StepLds l;
    std::memset(&l, 0, sizeof(l));
    // lists: one more tuple (and exponent) behind the last link - the far-away, zero-power stand-in an empty list slot reads
    const unsigned NL = (unsigned)N + (lists ? 1u : 0u);
    unsigned off = LDS_HEAD_BYTES + NL * 16u;
    l.aux = off; off += (unsigned)N * 4u;
    l.rx = off; if (lpt == 0) off += (unsigned)N * 8u;
    l.sinr = off; l.sh = off + (unsigned)N * 4u; if (reward_fn >= 2) off += (unsigned)N * 8u;
    off = (off + 7u) & ~7u;
    l.expo = off; if (mode == PL_POWER || mode == PL_SHADOW || mode == PL_POWK) off += NL * 8u;   // (head, tail) of -exponent / 2 per link (PL_POWK: (phi, 0))
    off = (off + 7u) & ~7u;
    l.lo = off; if (xpos) off += NL * 8u;                                            // low parts of (tx_x, tx_y) per link (exact positions)
    l.tflat = off; if (fuse_obs) off += (unsigned)N * 24u;
    off = (off + 15u) & ~15u;                            // the mask region is cleared with 16-byte stores
    l.mask = off;
    if (mask_words > 0) off += ((unsigned)R * mask_words + mask_words + (unsigned)R) * 4u;
    off = (off + 15u) & ~15u;
    // member lists: slots[R] (eight u16 link indices per RB, 0xFFFF = empty) then cnt[R] u32 (padded to 16 bytes) -
    // one contiguous region, (re)initialised with one 16-byte store per lane
    l.lists = off;
    if (lists) off += (unsigned)R * 16u + (((unsigned)R + 3u) & ~3u) * 4u;
    l.env_bytes = (off + 15u) & ~15u;
    return l;
}

// LDS of one env of the rollout kernel (byte offsets; StepLds): 0 ... 59 unused, 60 dump (u16) | 64 flags[4]: env flags, reward
// bits, ticket, pool count | 80 link[N + 1] tuples | expo[N + 1] (power law) | lo[N + 1] (exact positions) | slots[R + 1] (8 x u16)
// | cnt[R + 1] | pool[N] (rb, link) | 16 wave sums (the reward's group sums) | low[N + 1] (CueSinrShannon).  With two links per
// thread the region from 80 on becomes the env's table image.
StepLds rollout_lds_layout(int N, int R, int mode, int reward_fn, int xpos) {
    StepLds l;
    std::memset(&l, 0, sizeof(l));
    unsigned off = LDS_HEAD_BYTES + ((unsigned)N + 1u) * 16u;
    l.expo = off;
    if (mode == PL_POWER) off += ((unsigned)N + 1u) * 8u;
    else if (mode == PL_POWK) off += (((unsigned)N + 1u) * 4u + 7u) & ~7u;       // PL_POWK: the links' RBs (the tuple's fourth word holds phi)
    l.lo = off; if (xpos) off += ((unsigned)N + 1u) * 8u;        // exact positions: low parts of (tx_x, tx_y), + one for the stand-in
    off = (off + 15u) & ~15u;
    l.lists = off; off += ((unsigned)R + 1u) * 16u + (((unsigned)R + 1u + 3u) & ~3u) * 4u;
    l.pool = off; off += (unsigned)N * 8u;
    off = (off + 15u) & ~15u;
    l.aux = off; off += 64u;                                      // padded link counts: the waves' capacity sums (16 floats)
    l.rx = off;                                                   // CueSinrShannon: per link "a non-D2D link below the threshold" (+ one for the stand-in)
    if (reward_fn == D2D_REWARD_CUE_SINR_SHANNON) off += ((unsigned)N + 1u) * 4u;
    l.env_bytes = (off + 15u) & ~15u;
    return l;
}

// threads per env holding `lpt` links each, in whole waves
int threads_for(int N, int lpt) { return (((N + lpt - 1) / lpt + 63) / 64) * 64; }

}  // namespace

int plan_step(const StepInputs& in, StepPlan* out, const char** error) {
    const int N = in.N, R = in.R;
    const StepTuning& t = in.tune;
    if ((size_t)in.B * (size_t)N * 24 >= (1ull << 32)) {
        *error = "envs x links per GPU must stay below 2^32 / 24 (32-bit byte offsets in the step kernel)";
        return D2D_ERR_UNSUPPORTED;
    }
    const bool power_law = in.mode == PL_INV_SQUARE || in.mode == PL_POWER || in.mode == PL_POWK;
    const bool cue_sinr = in.reward_fn == D2D_REWARD_CUE_SINR_SHANNON;
    const bool rec_uniform = in.rec_uniform && t.srec != 0;

    // Small envs expand their LinearObs block inside the step launch, streamed by all threads of the workgroup - two launches of a
    // few microseconds each are bound by launch latency, not by HBM.  The fused expansion writes float32 only.
    const bool fuse = in.obs_mode == D2D_OBS_LINEAR && !in.obs_f64 && (t.fuse >= 0 ? t.fuse != 0 : N <= 128);
    const int fuse_obs = fuse ? ((6 * N) % 4 == 0 ? 4 : 2) : 0;

    // The rollout kernel (d2d_rollout.hip) serves: raw agent actions for every link or for all but a prefix with fixed actions,
    // any of the three rewards, one env per workgroup (64 ... 1024 links: a multiple of 64, or padded to the next one - measured
    // from 80 links up; no fused expansion), a power-law path loss.  Round 5: it is the faster one in every obs mode (same box,
    // 4096 x 512, r4 HEAD -> rollout: obs-less 21.3 -> 19.3 us, compact table 27.7 -> 25.8, with the decoded planes 28.3 -> 27.3,
    // profiles/r5_ab_rollout_kernel.jsonl; further since), so wherever it applies the lists are the default.
    const bool rollout_cfg = in.action_mode == 0 && (in.n_fixed == 0 || (in.n_fixed < N && in.col_mode == 0)) && in.bucketing &&
                             (in.reward_fn == D2D_REWARD_SYSTEM_CAPACITY || in.reward_fn == D2D_REWARD_SHANNON || cue_sinr) &&
                             !fuse && power_law && (t.ablate & ~8192) == 0 && t.prefetch != 0 && t.threads == 0 && t.epw <= 1 &&
                             t.block == 0 && (N % 64 == 0 || N > 64) && N <= 1024;
    // Per-RB member lists only where they can hold the env: with more than four links per RB on average a ninth link on some RB
    // is the rule, the list build is wasted and the workgroup sweeps all pairs anyway (N > 8 R: by pigeonhole), so those shapes
    // go straight to the masks or the sweep.
    const bool lists_can_help = (long long)N <= 4ll * R;
    const bool lists_pay = lists_can_help && (N > 1024 || in.obs_mode == D2D_OBS_NONE || rollout_cfg);
    const int walk_asked = t.walk >= 0 ? t.walk : (lists_pay ? 2 : 0);
    const bool rollout_wanted = in.bucketing && walk_asked == 2 && rollout_cfg && in.col_mode == 0;

    // ---- the generic kernels (d2d_step.hip).  lpt = links per thread held in registers (1 or 2; 0 = strided beyond 2 x 1024
    // links), tpe = threads per env (one per link up to 1024)
    int lpt, tpe;
    if (t.threads > 0) {
        tpe = t.threads;
        lpt = N <= tpe ? 1 : (N <= 2 * tpe ? 2 : 0);
    } else {
        const int want = t.lpt > 0 ? t.lpt : 1;
        lpt = threads_for(N, want) <= 1024 ? want : (threads_for(N, 2) <= 1024 ? 2 : 0);
        tpe = lpt ? threads_for(N, lpt) : 1024;
    }
    // per-RB membership masks: u32 words, every link of the env in some thread's registers, N <= 1024 (the 32-bit summary word names
    // up to 32 mask words).  Per-RB member lists (walk 2): any N whose links sit in registers; an env that overflows a list falls
    // back to the masks when they exist, else to the all-pairs sweep.  (The rollout kernel has its own way with CueSinrShannon; the
    // generic kernels' lists have none.)
    const bool lists_asked = in.bucketing && walk_asked == 2 && lpt > 0 && !cue_sinr;
    const auto env_bytes = [&](int W, int lists) { return step_lds_layout(N, R, W, fuse_obs, lpt, in.reward_fn, in.mode, lists, in.xpos).env_bytes; };
    const int words = (N + 31) / 32;
    const int W = in.bucketing && lpt > 0 && N <= 1024 && env_bytes(words, lists_asked) <= 96 * 1024 ? words : 0;
    // masks that do not fit (thousands of RBs): the lists are 20 bytes per RB instead of 4 per RB and 32 links - take them when
    // nobody chose a search variant
    const bool lists_instead = W == 0 && !lists_asked && lists_can_help && t.walk < 0 && in.bucketing && lpt > 0 && !cue_sinr;
    const bool lists = (lists_asked || lists_instead) && env_bytes(W, 1) <= 96 * 1024;
    const int walk = lists ? 2 : (lists_asked || lists_instead || (walk_asked == 2 && !rollout_wanted)) ? 0 : walk_asked;

    // ---- the rollout kernel: no masks, its own LDS layout (17 KB per env at 512 links on 256 RBs).  One link per thread, or two
    // ADJACENT ones (links 2t and 2t + 1, N / 2 threads per env): every per-wave instruction - the scalar record load, barriers,
    // ballots, the wave reduction, the ticket - is paid once per 128 links, half as many waves are launched, and a thread's two
    // results are one 8-byte element of every plane and 48 contiguous bytes of the table.  Two wherever the device classes fill
    // aligned groups of 128 links (one scalar record load serves the wave; per-lane records for two links push the kernel past 64
    // VGPRs).  Same box, 4096 x 512: obs-less 20.2 -> 19.0 us, compact table 26.7 -> 24.5 (profiles/r5_table_rows_through_lds.jsonl).
    // (Other exponents - the power-law kernel, twice the arithmetic per pair - gain nothing from two: COST-Hata obs-less 32.0 us
    // with one link per thread, 33.4 with two; table 37.3 / 37.8.)  Fixed actions live in per-link records, CueSinrShannon takes a
    // second look at the RB's members and exact positions add a fourth 16-byte row per link: one link per thread for each.
    const bool two_asked = (t.lpt > 0 ? t.lpt == 2 : in.rec_uniform128 && rec_uniform && in.mode == PL_INV_SQUARE) && N % 128 == 0;
    const int ro_lpt = two_asked && in.n_fixed == 0 && !cue_sinr && !in.xpos ? 2 : 1;
    const StepLds ro_lds = rollout_lds_layout(N, R, in.mode, in.reward_fn, in.xpos);
    const bool rollout = rollout_wanted && ro_lds.env_bytes <= 64 * 1024;

    StepPlan& p = *out;
    std::memset(&p, 0, sizeof(p));
    p.rollout = rollout;
    p.walk = walk;
    p.fuse_obs = fuse_obs;
    p.lpt = rollout ? ro_lpt : lpt;
    p.tpe = rollout ? threads_for(N, ro_lpt) : tpe;
    p.mask_words = rollout ? 0 : W;
    p.lds = rollout ? ro_lds : step_lds_layout(N, R, W, fuse_obs, lpt, in.reward_fn, in.mode, lists, in.xpos);
    // scalar record loads: per-lane records where two links per thread were asked for on records that are not uniform per 128,
    // and with fixed actions (decided wherever the rollout kernel is wanted, whether or not its LDS fits)
    p.rec_uniform = rollout_wanted ? rec_uniform && in.n_fixed == 0 && (!two_asked || in.rec_uniform128) : rec_uniform;
    // nontemporal result stores: never with LinearObs (the expansion kernel reads the table right behind this launch).  In the
    // generic kernels no consistent gain (profiles/r3_ab_*): off unless asked for.  The rollout kernel takes them by default:
    // interleaved in one process at 4096 x 512, obs-less 17.98 -> 17.51 us, compact table 25.11 -> 24.76
    // (profiles/r5_rollout_nt_and_links_per_thread.jsonl)
    p.nt_results = in.obs_mode != D2D_OBS_LINEAR && (t.nt > 0 || (rollout && t.nt < 0));
    const size_t env_lds = p.lds.env_bytes;
    if (env_lds > 160 * 1024) {
        *error = "links per env exceed the LDS staging capacity";
        return D2D_ERR_UNSUPPORTED;
    }
    // envs per workgroup: small envs share one (N = 50: four 64-thread envs in 256 threads)
    int epw = rollout ? 1 : (t.epw > 0 ? t.epw : (p.tpe >= 256 ? 1 : 256 / p.tpe));
    if (epw > in.B) epw = in.B;
    while (epw > 1 && ((size_t)epw * env_lds > 64 * 1024 || epw * p.tpe > 1024)) --epw;
    p.epw = epw;
    // more store streams per env for the fused obs phase
    const int threads = epw * p.tpe;
    p.block = t.block > 0 ? (t.block > threads ? t.block : threads) : (fuse && threads < 256 ? 256 : threads);
    if (p.block > 1024) {
        *error = "step workgroup exceeds 1024 threads";
        return D2D_ERR_INVALID;
    }
    // action prefetch distance = the envs resident on the chip at once (LDS: 160 KB / CU, threads: 2048 / CU), as a multiple of
    // 8 workgroups so that the prefetching and the consuming workgroup share an XCD (and its L2)
    int per_cu = (int)((160 * 1024) / ((size_t)epw * env_lds ? (size_t)epw * env_lds : 1));
    if (per_cu > 2048 / p.block) per_cu = 2048 / p.block;
    if (per_cu < 1) per_cu = 1;
    const int dist = t.prefetch >= 0 ? t.prefetch : per_cu * in.num_cus * epw;
    p.prefetch_envs = dist - dist % (8 * epw);
    p.tpe_magic = ((1u << 20) + (unsigned)p.tpe - 1) / (unsigned)p.tpe;
    if (fuse) {
        p.obs_rotate = t.obs_rotate >= 0 ? t.obs_rotate : 29;
        p.obs_q_per_row = (unsigned)(6 * N / fuse_obs);
        p.obs_q_magic = ((1ull << 40) + p.obs_q_per_row - 1) / p.obs_q_per_row;
    }
    p.grid = (unsigned)((in.B + epw - 1) / epw);
    p.lds_bytes = env_lds * (size_t)epw;
    p.obs_expand = in.obs_mode == D2D_OBS_LINEAR && !fuse;

    // ---- the kernel's template arguments
    StepKernel& k = p.kernel;
    k.mode = in.mode;
    k.rollout = rollout;
    const int nt = p.nt_results ? OPT_NT : 0, srec = p.rec_uniform ? OPT_SREC : 0, xp = in.xpos ? OPT_XPOS : 0;
    if (rollout) {                                       // a link count that is no multiple of 64: padded, per-lane records
        k.lpt = ro_lpt;
        k.opt = (N % 64 ? nt | OPT_PAD : srec | nt) | xp;
        return D2D_OK;
    }
    const bool full = lpt > 0 && epw == 1 && N == lpt * p.tpe && p.block == p.tpe && !fuse;
    const bool hot_common = power_law && in.action_mode == 0 && in.col_mode == 0 && in.reward_fn == D2D_REWARD_SYSTEM_CAPACITY &&
                            p.prefetch_envs > 0 && (t.ablate & 8191) == 0 && W > 0 && !in.xpos;
    // HOT level 1: the rollout configuration with the masks (dense occupancy), one env per workgroup, no lane predication
    const bool hot1 = hot_common && in.n_fixed == 0 && (walk == 0 || lists) && lpt == 1 && full;
    // HOT level 2: several small envs per workgroup with the 16-byte fused LinearObs expansion (BASELINE config 2), a fixed
    // prefix (traffic-model CUEs) allowed
    const bool hot2 = hot_common && in.n_fixed < N && walk == 0 && fuse_obs == 4 && lpt == 1 && !full;
    k.lpt = lpt;
    k.full = full;
    k.hot = hot1 ? 1 : (hot2 ? 2 : 0);
    k.opt = hot1 ? srec | nt : (hot2 ? 0 : (lists ? OPT_LISTS : 0) | xp);
    return D2D_OK;
}

namespace {

// The store policy of the obs stream where nobody set one (ObsTuning::nt < 0).  `one_trip`: a flat kernel that stages T[env] with
// 16-byte loads in one round trip (6N % 4 == 0).  Under the write-through policy (5, sc1 nt) a store is acknowledged by memory,
// not by L2, so the kernel is bound by how long a workgroup lives and not by HBM.  With the 8-byte staging loop of rounds 1-6
// (two dependent L2 trips for half the waves, the kernel arguments fetched in two scalar trips around a division, the index
// arithmetic behind the barrier) waves lived 1324 quad-cycles under 5 against 1114 under 1 and the kernel lost 10 %
// (profiles/r7_pmc_obs_wave_lifetime.json).  With everything ahead of the first store shortened, 5 is the faster one at two
// pieces per workgroup (profiles/r7_obs_staging_sweep.jsonl, one box: float32 1024 x 2 3756 -> 3581 us, float64 7417 -> 7131)
// and mixed at three and four, where more bytes in flight per CU hide a longer life (ahead at 1024 x 3 and x 4 in float32, behind
// at 512 x 3, 512 x 4 and float64 1024 x 3): those shapes are set by hand and keep 1 unless the policy is set too.  (Rounds
// 4-6 gave "its table rows are re-read through the same L2" as the reason for the loss; the probe's staged fill re-reads a row of
// the same size through the same L2 and GAINS from 5.)  The row-aligned kernels and the 8-byte staging of odd N keep 1.
int obs_store_policy(int nt, bool one_trip, int pieces) { return nt >= 0 ? nt : (one_trip && pieces <= 2 ? 5 : 1); }

// ObsArgs::chunk_magic of a flat launch: block / chunks (block / 8 / chunks with the XCD grouping) as a multiply-shift by
// M = ceil(2^40 / chunks), exact while n x chunks < 2^40 (the error n (M chunks - 2^40) / (chunks 2^40) stays below 1 / chunks) and
// n < 2^24 keeps n M inside 64 bits; a grid beyond that divides (0).
unsigned long long obs_chunk_magic(const ObsArgs& o) {
    const unsigned long long grid = (unsigned long long)o.B * (unsigned)o.chunks, n = o.xcd_remap ? grid / 8 : grid, d = (unsigned)o.chunks;
    return n < (1ull << 24) && n * d < (1ull << 40) ? ((1ull << 40) + d - 1) / d : 0;
}

}  // namespace

// LinearObs expansion launch geometry for a [B, N, 6] table (shared by the step path and d2d_expand_table).
ObsArgs plan_obs(const ObsTuning& t, int B, int N, int out_f64) {
    ObsArgs o;
    std::memset(&o, 0, sizeof(o));
    o.B = B; o.N = N;
    o.out_f64 = out_f64;
    if (out_f64 && t.variant != 3) {
        // float64 block (d2d_set_obs_dtype): flat slabs of double2 pieces - one aligned float2 of T each, 3N per row, any N
        o.vec = 2;
        o.q_per_row = (unsigned)(3 * N);
        o.q_magic = ((1ull << 40) + o.q_per_row - 1) / o.q_per_row;
        // (1024 x 2 as in float32: with the single-trip staging still ahead of 512 x 2, 7131 against 7181 us, r7_obs_staging_sweep.jsonl)
        const bool one_trip = (6 * N) % 4 == 0;
        o.block = t.block > 0 ? t.block : 1024;
        int passes = t.rows > 0 ? t.rows : 2;
        if (passes > 4) passes = 4;
        o.rows_per_wg = passes;
        const unsigned total = (unsigned)N * o.q_per_row, slab = (unsigned)passes * (unsigned)o.block;
        o.chunks = (int)((total + slab - 1) / slab);
        o.xcd_remap = (t.xcd > 0 && B % 8 == 0) ? 1 : 0;
        o.nontemporal = obs_store_policy(t.nt, one_trip, passes);
        o.variant = 2;
        o.chunk_magic = obs_chunk_magic(o);
        return o;
    }
    o.vec = (6 * N) % 4 == 0 ? 4 : 2;
    o.q_per_row = (unsigned)(6 * N / o.vec);
    o.q_magic = ((1ull << 40) + o.q_per_row - 1) / o.q_per_row;
    // Launch geometry.  Round 4 (tools/probes/obs_policy_geometry.py, MI355X, N = 512): FLAT slabs - the env's [N][6N] block as one
    // flat array of float4, a 1024-thread workgroup writing two consecutive 16 KB pieces of it whatever the row length - the
    // shape of the fastest fill of the probe family: 7.21 TB/s against 7.01 for the row-aligned shape of rounds 1-3 (768 threads
    // = one row's float4 count, two 12 KB rows per workgroup) in interleaved rounds on one box; 3 or 4 pieces and 768- or 512-thread
    // slabs are slower (round 7, with T staged in one trip: still so, and the store policy is obs_store_policy's).  Rounds 1-3 (tools/tune_obs.py): among row-aligned shapes the fastest
    // is the one where every thread issues exactly TWO 16-B stores (6.96 TB/s vs 5.9 for 96-KiB slabs and 5.6 for 786-KiB slabs):
    // small slabs dispatched in order keep the chip-wide write front nearly sequential in address, and a workgroup never
    // outlives its neighbours.  D2D_TUNE_OBS_VARIANT = 3 keeps the row-aligned kernel (A/B, and 8-byte rows when 6N % 4 != 0).
    const bool flat = o.vec == 4 && (t.variant == 0 || t.variant == 2) && !out_f64;
    int block = t.block;
    if (block <= 0) {
        block = flat ? 1024 : (int)((o.q_per_row + 63) / 64) * 64;
        if (block < 256) block = 256;
        if (block > 1024) block = 1024;
    }
    int rows = t.rows;
    if (rows <= 0) {
        rows = flat ? 2 : (int)((2u * (unsigned)block + o.q_per_row / 2) / o.q_per_row);
        if (rows < 1) rows = 1;
    }
    if (rows > N && !flat) rows = N;
    o.rows_per_wg = rows;
    o.chunks = (N + rows - 1) / rows;
    if (flat) {                                          // `rows` = consecutive pieces of `block` float4 per workgroup (at most 4)
        if (rows > 4) rows = 4;
        o.rows_per_wg = rows;
        const unsigned total = (unsigned)N * o.q_per_row, slab = (unsigned)rows * (unsigned)block;
        o.chunks = (int)((total + slab - 1) / slab);
    }
    o.xcd_remap = (t.xcd > 0 && B % (8 * t.xcd) == 0) ? t.xcd : 0;   // envs interleaved per XCD
    o.nontemporal = obs_store_policy(t.nt, flat, o.rows_per_wg);
    o.block = block;
    // tune_variant 2 names the flat kernel, whose grid is sized in flat chunks: when the flat shape does not apply (8-byte rows, a
    // float64 block's float32 consumers) the row-aligned default runs on the row-aligned geometry computed above
    o.variant = flat ? 2 : (t.variant == 2 ? 0 : t.variant);
    o.stagger = t.stagger;
    if (flat) o.chunk_magic = obs_chunk_magic(o);
    return o;
}

}  // namespace d2d
