// libd2d_mobility.so (include/d2d_mobility.h): one Gauss-Markov move of every device of every env, one launch.  gfx950.
//
// Shape: reset_kernel's (d2d_reset.hip) - one thread per (env, placement unit): the base station, a CUE, or a DUE PAIR, whose thread
// moves the transmitter and then tethers the receiver to where it now stands, so the tether needs no synchronisation.  About 32 bytes
// per device (position and velocity, read and written) against two Philox4x32-10 Gaussians per device: no LDS, no scratch, plain
// loads and stores, every word written by the one thread that owns it.  The arithmetic is spelled as fmaf, so that the lockstep and
// the per-env clock - one kernel, one code path behind the clock - and every compiler version give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "d2d_addon.h"
#include "d2d_mobility.h"
#include "d2d_step_device.h"

namespace {

struct MoveArgs {
    float* pos_x;
    float* pos_y;
    float* vel_x;
    float* vel_y;
    const unsigned char* fixed;     // [D] or null
    const int* elapsed_env;         // per-env clock (reset_env != null), else the scalars step / episode
    int* start_env;
    const unsigned* episode_env;
    const int* reset_env;
    int D, C;
    unsigned units;                 // placement units per env: base station + C CUEs + P DUE pairs
    unsigned units_magic;           // floor(2^32 / units)
    unsigned total;                 // n_envs * units
    unsigned first_env, seed_lo, seed_hi, step, episode;
    float memory, noise_scale, speed_std, dt;
    float cell_r, d2d_r, d2d_in;    // d2d_in = d2d_r - ulp(cell_r): where a tethered device is put
};

struct Clock {
    unsigned env, episode, t;       // counter words 0 - 2
};

__device__ __forceinline__ float2 normals(const MoveArgs& a, const Clock& c, unsigned d) {
    return make_float2(d2d::philox_normal(c.env, c.episode, c.t, 2u * d, a.seed_lo, a.seed_hi),
                       d2d::philox_normal(c.env, c.episode, c.t, 2u * d + 1u, a.seed_lo, a.seed_hi));
}

// p onto the circle of radius `target` around c if it stands further than `limit` from it
__device__ __forceinline__ bool pull_inside(float2& p, float2 c, float limit, float target) {
    const float dx = p.x - c.x, dy = p.y - c.y;
    const float d = sqrtf(fmaf(dx, dx, dy * dy));
    if (!(d > limit)) return false;
    const float f = target / d;
    p = make_float2(fmaf(dx, f, c.x), fmaf(dy, f, c.y));
    return true;
}

// Device d (flat index k) at clock c; `anchor` is what it is tethered to, if it is.  Returns where it stands afterwards.
__device__ __forceinline__ float2 move_device(const MoveArgs& a, const Clock& c, size_t k, unsigned d, bool fixed, bool tethered,
                                              float2 anchor) {
    if (c.t == 0u) {                                                     // start of the episode: the stationary distribution
        float2 v = make_float2(0.f, 0.f);
        if (!fixed) { const float2 n = normals(a, c, d); v = make_float2(a.speed_std * n.x, a.speed_std * n.y); }
        a.vel_x[k] = v.x; a.vel_y[k] = v.y;
        return v;                                                        // (nobody reads a position at t == 0)
    }
    float2 p = make_float2(a.pos_x[k], a.pos_y[k]);
    if (fixed) return p;
    const float2 n = normals(a, c, d);
    float2 v = make_float2(fmaf(a.memory, a.vel_x[k], a.noise_scale * n.x), fmaf(a.memory, a.vel_y[k], a.noise_scale * n.y));
    p = make_float2(fmaf(v.x, a.dt, p.x), fmaf(v.y, a.dt, p.y));
    bool flip = tethered && pull_inside(p, anchor, a.d2d_r, a.d2d_in);
    const bool wall = pull_inside(p, make_float2(0.f, 0.f), a.cell_r, a.cell_r);
    if (tethered && wall) pull_inside(p, anchor, a.d2d_r, a.d2d_in);     // the wall's rounding may have parted the pair again
    flip ^= wall;
    a.pos_x[k] = p.x; a.pos_y[k] = p.y;
    a.vel_x[k] = flip ? -v.x : v.x; a.vel_y[k] = flip ? -v.y : v.y;
    return p;
}

__global__ __launch_bounds__(256) void mobility_move_kernel(const MoveArgs a) {
    const unsigned gid = blockIdx.x * 256u + threadIdx.x;
    if (gid >= a.total) return;
    unsigned b = __umulhi(gid, a.units_magic);                           // gid / units: the estimate is exact or one short
    unsigned u = gid - b * a.units;
    if (u >= a.units) { u -= a.units; ++b; }
    Clock c;
    c.env = a.first_env + b;
    if (a.reset_env) {
        const unsigned next = a.episode_env[b];
        if (a.reset_env[b] != 0) {
            c.episode = next; c.t = 0u;
            if (u == 0u) a.start_env[b] = 0;                             // read by envs that move only: never by this env in this launch
        } else {
            c.episode = next - 1u; c.t = (unsigned)(a.elapsed_env[b] - a.start_env[b]) + 1u;
        }
    } else {
        c.episode = a.episode; c.t = a.step;
    }
    const size_t base = (size_t)b * (size_t)a.D;
    const float2 none = make_float2(0.f, 0.f);
    if (u <= (unsigned)a.C) {                                            // the base station (never moves) or a CUE
        move_device(a, c, base + u, u, u == 0u || (a.fixed && a.fixed[u]), false, none);
        return;
    }
    const unsigned d = (unsigned)a.C + 1u + 2u * (u - (unsigned)a.C - 1u);   // transmitter; its receiver is d + 1
    const bool fix_tx = a.fixed && a.fixed[d], fix_rx = a.fixed && a.fixed[d + 1u];
    float2 rx = none;
    if (fix_rx && !fix_tx && c.t != 0u) rx = make_float2(a.pos_x[base + d + 1u], a.pos_y[base + d + 1u]);
    const float2 tx = move_device(a, c, base + d, d, fix_tx, fix_rx && !fix_tx, rx);
    move_device(a, c, base + d + 1u, d + 1u, fix_rx, true, tx);
}

}  // namespace

extern "C" int d2d_mobility_move(float* pos_x, float* pos_y, float* vel_x, float* vel_y, const uint8_t* fixed_mask, int64_t n_envs,
                                 int32_t n_cues, int32_t n_due_pairs, uint64_t first_env, uint64_t seed, float memory,
                                 float noise_scale, float speed_std, float dt_s, float cell_radius_m, float d2d_radius_m, uint32_t step,
                                 uint32_t episode, const int32_t* elapsed_env, int32_t* start_env, const uint32_t* episode_env,
                                 const int32_t* reset_env, void* hip_stream) try {
    if (n_envs < 0 || n_envs > 0x7FFFFFFFll) return fail("n_envs must be in [0, 2^31)");
    if (n_cues < 0 || n_due_pairs < 0 || n_cues > (1 << 24) || n_due_pairs > (1 << 24)) return fail("n_cues and n_due_pairs must be in [0, 2^24]");
    if (first_env + (uint64_t)n_envs > (1ull << 32)) return fail("first_env + n_envs must not exceed 2^32 (the env counter word)");
    if (!(memory >= 0.0f && memory < 1.0f)) return fail("memory must be in [0, 1)");
    if (!(noise_scale >= 0.0f) || !(speed_std >= 0.0f) || !std::isfinite(noise_scale) || !std::isfinite(speed_std) || !std::isfinite(dt_s))
        return fail("noise_scale and speed_std must be finite and >= 0, dt_s finite");
    if (!(cell_radius_m > 0.0f) || !std::isfinite(cell_radius_m)) return fail("cell_radius_m must be finite and > 0");
    const float grid = std::nextafterf(cell_radius_m, HUGE_VALF) - cell_radius_m;             // ulp(cell_radius_m)
    if (!(d2d_radius_m > grid) || !std::isfinite(d2d_radius_m)) return fail("d2d_radius_m must be finite and > ulp(cell_radius_m)");
    if (!pos_x || !pos_y || !vel_x || !vel_y) return fail("null device pointer");
    if (reset_env && (!elapsed_env || !start_env || !episode_env)) return fail("the per-env clock needs elapsed_env, start_env and episode_env");
    if (n_envs == 0) return 0;
    MoveArgs a;
    a.pos_x = pos_x; a.pos_y = pos_y; a.vel_x = vel_x; a.vel_y = vel_y; a.fixed = fixed_mask;
    a.elapsed_env = elapsed_env; a.start_env = start_env; a.episode_env = episode_env; a.reset_env = reset_env;
    a.C = n_cues; a.D = 1 + n_cues + 2 * n_due_pairs;
    a.units = 1u + (unsigned)n_cues + (unsigned)n_due_pairs;
    a.units_magic = a.units == 1u ? 0xFFFFFFFFu : (unsigned)(0x100000000ull / a.units);       // one short at most: the kernel corrects
    const unsigned long long total = (unsigned long long)n_envs * a.units;
    if (total >= 0xFFFFFF00ull) return fail("n_envs * (1 + n_cues + n_due_pairs) must stay below 2^32 - 256");
    a.total = (unsigned)total;
    a.first_env = (unsigned)first_env;
    a.seed_lo = (unsigned)(seed & 0xFFFFFFFFull); a.seed_hi = (unsigned)(seed >> 32);
    a.step = step; a.episode = episode;
    a.memory = memory; a.noise_scale = noise_scale; a.speed_std = speed_std; a.dt = dt_s;
    a.cell_r = cell_radius_m; a.d2d_r = d2d_radius_m; a.d2d_in = d2d_radius_m - grid;
    hipLaunchKernelGGL(mobility_move_kernel, dim3((a.total + 255u) / 256u), dim3(256), 0, static_cast<hipStream_t>(hip_stream), a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(std::string("mobility_move_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

D2D_ADDON_LAST_ERROR(d2d_mobility_last_error)
