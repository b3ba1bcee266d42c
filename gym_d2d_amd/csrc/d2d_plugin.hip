// libd2d_plugin.so (include/d2d_plugin.h): the counter-based normal generator behind ArrayPathLoss's view.normal().  gfx950.
//
// A streaming write: Philox4x32-10 + Box-Muller per element (philox_normal, d2d_step_device.h - the step kernel's own shadowing
// draw, not a copy of it), 16 bytes per lane per store (two float64 or four float32 consecutive elements), a grid of about 32
// workgroups per CU striding over the block as launch_gain_from_db does.  A lane decomposes its first flat index into (env, row,
// column) once per vector and walks the rest by increments; 32-bit divisions while the block has fewer than 2^32 elements
// (4096 x 512 x 512 has 1.07e9).
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>

#include "d2d_addon.h"
#include "d2d_plugin.h"
#include "d2d_step_device.h"

namespace {

struct NormalArgs {
    unsigned long long total;     // n_envs * n_rows * n_cols
    unsigned n_rows, n_cols;
    unsigned first_env, step, kind, seed_lo, seed_hi;
    int narrow;                   // total < 2^32: 32-bit index arithmetic
};

template <class T>
__device__ __forceinline__ T normal_at(const NormalArgs& a, unsigned b, unsigned r, unsigned c) {
    const unsigned ctr2 = a.kind == 0u ? (r | (c << 16)) : (c | (c << 16));
    return (T)d2d::philox_normal(a.first_env + b, a.step, ctr2, a.kind, a.seed_lo, a.seed_hi);
}

template <class T>
__global__ __launch_bounds__(256) void normal_kernel(T* __restrict__ out, const NormalArgs a) {
    constexpr unsigned VEC = 16u / sizeof(T);
    using V = typename std::conditional<sizeof(T) == 8, double2, float4>::type;
    const unsigned long long nvec = a.total / VEC;
    const unsigned long long stride = (unsigned long long)gridDim.x * 256u;
    for (unsigned long long v = (unsigned long long)blockIdx.x * 256u + threadIdx.x; v < nvec; v += stride) {
        const unsigned long long k0 = v * VEC;
        unsigned b, r, c;
        if (a.narrow) {
            const unsigned k = (unsigned)k0, q = k / a.n_cols;
            c = k - q * a.n_cols; b = q / a.n_rows; r = q - b * a.n_rows;
        } else {
            const unsigned long long q = k0 / a.n_cols;
            c = (unsigned)(k0 - q * a.n_cols); b = (unsigned)(q / a.n_rows); r = (unsigned)(q - (unsigned long long)b * a.n_rows);
        }
        T x[VEC];
#pragma unroll
        for (unsigned e = 0; e < VEC; ++e) {
            x[e] = normal_at<T>(a, b, r, c);
            if (++c == a.n_cols) { c = 0; if (++r == a.n_rows) { r = 0; ++b; } }
        }
        V w;
        if constexpr (sizeof(T) == 8) w = make_double2(x[0], x[1]);
        else w = make_float4(x[0], x[1], x[2], x[3]);
        reinterpret_cast<V*>(out)[v] = w;
    }
    // the tail of fewer than VEC elements: one lane of the first workgroup
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (unsigned long long k = nvec * VEC; k < a.total; ++k) {
            const unsigned long long q = k / a.n_cols;
            const unsigned c = (unsigned)(k - q * a.n_cols), b = (unsigned)(q / a.n_rows), r = (unsigned)(q - (unsigned long long)b * a.n_rows);
            out[k] = normal_at<T>(a, b, r, c);
        }
    }
}

int device_cus(int dev) {
    static std::mutex mu;
    static int cus[64] = {0};
    if (dev < 0 || dev >= 64) return 256;
    std::lock_guard<std::mutex> lock(mu);
    if (cus[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) { (void)hipGetLastError(); n = 256; }
        cus[dev] = n;
    }
    return cus[dev];
}

}  // namespace

extern "C" int d2d_plugin_normal(void* out_dev, int32_t dtype, int64_t n_envs, uint64_t first_env, int32_t n_rows, int32_t n_cols,
                                 uint64_t step, int32_t kind, uint64_t seed, void* hip_stream) try {
    if (!out_dev) return fail("null out_dev");
    if (dtype != D2D_PLUGIN_F32 && dtype != D2D_PLUGIN_F64) return fail("dtype must be D2D_PLUGIN_F32 or D2D_PLUGIN_F64");
    if (kind != 0 && kind != 1) return fail("kind must be 0 or 1");
    if (n_envs < 0 || n_rows < 1 || n_cols < 1 || n_rows > 65536 || n_cols > 65536) return fail("n_envs >= 0, 1 <= n_rows, n_cols <= 65536");
    if (kind == 1 && n_rows != 1) return fail("kind 1 (own-link draws) takes n_rows == 1");
    if (first_env + (uint64_t)n_envs > (1ull << 32)) return fail("first_env + n_envs must not exceed 2^32 (the env counter word)");
    if (n_envs == 0) return 0;
    if (reinterpret_cast<uintptr_t>(out_dev) % 16 != 0) return fail("out_dev must be 16-byte aligned");
    int dev = 0;
    hipPointerAttribute_t attr;
    hipError_t e = hipPointerGetAttributes(&attr, out_dev);
    if (e != hipSuccess) (void)hipGetLastError();
    if (e != hipSuccess || (attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeManaged)) return fail("out_dev must be device or managed memory");
    if (hipGetDevice(&dev) != hipSuccess || dev != attr.device) return fail("out_dev must live on the current HIP device");
    NormalArgs a;
    a.total = (unsigned long long)n_envs * (unsigned long long)n_rows * (unsigned long long)n_cols;
    a.n_rows = (unsigned)n_rows; a.n_cols = (unsigned)n_cols;
    a.first_env = (unsigned)first_env; a.step = (unsigned)step; a.kind = (unsigned)kind;
    a.seed_lo = (unsigned)(seed & 0xFFFFFFFFull); a.seed_hi = (unsigned)(seed >> 32);
    a.narrow = a.total < (1ull << 32);
    const unsigned vec = dtype == D2D_PLUGIN_F64 ? 2u : 4u;
    unsigned long long blocks = (a.total / vec + 255) / 256;
    const unsigned long long cap = (unsigned long long)device_cus(dev) * 32;
    if (blocks > cap) blocks = cap;
    if (blocks == 0) blocks = 1;                                  // fewer elements than one vector: the tail lane alone
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (dtype == D2D_PLUGIN_F64) hipLaunchKernelGGL(normal_kernel<double>, dim3((unsigned)blocks), dim3(256), 0, s, static_cast<double*>(out_dev), a);
    else hipLaunchKernelGGL(normal_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, s, static_cast<float*>(out_dev), a);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(std::string("normal_kernel launch: ") + hipGetErrorString(e));
    return 0;
} D2D_ADDON_CATCH

D2D_ADDON_LAST_ERROR(d2d_plugin_last_error)
