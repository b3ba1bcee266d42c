// The host half of a side library (libd2d_<name>.so, one translation unit each): the per-thread error slot behind
// d2d_<name>_last_error(), the catch tail of an exported call, the launch that lifts the dynamic-LDS limit, and the argument checks
// the law-taking libraries share.  Everything here has internal linkage - a library exports what its public header declares and
// nothing else.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

namespace {

thread_local std::string g_addon_error;

int fail(const std::string& msg) {
    try { g_addon_error = msg; } catch (...) { }
    return 1;
}

// extern "C" int d2d_x(...) try { ... } D2D_ADDON_CATCH
#define D2D_ADDON_CATCH                                                     \
    catch (const std::exception& ex) { return fail(ex.what()); }            \
    catch (...) { return fail("unknown exception"); }

#define D2D_ADDON_LAST_ERROR(fn) extern "C" const char* fn(void) { return g_addon_error.c_str(); }

// the values of every library's D2D_*_LAW_* macros (each .hip asserts its own against these)
constexpr int32_t LAW_INV_SQUARE = 0, LAW_POWER = 1, LAW_POW_K = 2;

// one kernel launch; more than 64 KiB of dynamic LDS has to be asked for first
template <typename Args>
hipError_t launch(void (*kernel)(Args), dim3 grid, dim3 block, unsigned lds, hipStream_t s, const Args& a) {
    if (lds > 64u * 1024u) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, grid, block, lds, s, a);
    return hipGetLastError();
}

// The shared refusals, in the order every library states them; the message, or null.  A library without an RB dimension passes
// max_rbs = 0.  The two are apart because some libraries check arguments of their own between the sizes and the law.
const char* check_sizes(int64_t n_envs, int32_t n_links, int max_links, int32_t n_rbs, int max_rbs, int32_t n_dev) {
    thread_local std::string why;
    if (n_envs < 0 || n_envs > 0x7FFFFFFFll) return "n_envs must be in [0, 2^31)";
    if (n_links < 1 || n_links > max_links) return (why = "n_links must be in [1, " + std::to_string(max_links) + "]").c_str();
    if (max_rbs && (n_rbs < 1 || n_rbs > max_rbs)) return (why = "n_rbs must be in [1, " + std::to_string(max_rbs) + "]").c_str();
    if (n_dev < 1) return "n_dev must be >= 1";
    return nullptr;
}

const char* check_law(int32_t law, int32_t pow_k) {
    if (law != LAW_INV_SQUARE && law != LAW_POWER && law != LAW_POW_K) return "unknown law";
    if (law == LAW_POW_K && (pow_k < 1 || pow_k > 8)) return "pow_k must be in [1, 8]";
    return nullptr;
}

}  // namespace
