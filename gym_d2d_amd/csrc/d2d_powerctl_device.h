// What the two kernels that run the target-SINR power iteration out of LDS share (d2d_powerctl.hip: one target; d2d_balance.hip: a
// search over targets): a slot's SINR under a vector of linear powers, on the same operands in the same order in both, so a probe of
// the search sees power_control()'s values bit for bit.  The LDS layout stays each kernel's own: `L` is its struct of array
// pointers, of which this reads tx, rxa, rxb and hh.  (The update of one power is restated in d2d_balance.hip: hoisted here it
// changed the instruction schedule of powerctl_kernel, and that kernel stays as it was compiled before.)
#pragma once

#include <hip/hip_runtime.h>

#include "d2d_step_device.h"

namespace d2d {

constexpr unsigned PC_NO_RB = 0x80000000u;                       // range word of a link on no RB

// sinr_db of the link in slot k under the linear powers z, as the step forms it; the caller has checked that the link is on an RB.
// range = first slot of the link's RB group | (last + 1) << 16
template <int MODE, typename L>
__device__ __forceinline__ float slot_sinr_db(const L& s, const float* z, int k, unsigned range, int pow_k) {
    constexpr bool POWLAW = MODE != PL_INV_SQUARE;
    const float4 rx = s.rxa[k];                                          // rx x, rx y, rx_pl, noise
    const float2 own = s.rxb[k];                                         // own-pair gain, rx_lin
    const float sig = z[k] * own.x * rx.z * own.y;                       // simulator.py:93
    const int q_end = (int)(range >> 16);
    double acc = 0.0;
    for (int q = (int)(range & 0xFFFFu); q < q_end; ++q) {
        const float4 o = s.tx[q];
        const float dx = o.x - rx.x, dy = o.y - rx.y;
        const float d2 = fmaf(dx, dx, dy * dy);
        const float g = pair_gain<MODE>(d2, POWLAW ? s.hh[q] : make_float2(-1.0f, 0.0f), pow_k);
        const float term = z[q] * g;                                     // simulator.py:97-101, linear mW
        acc += q != k ? (double)term : 0.0;                              // j != i: slots and links correspond one to one
    }
    const float accf = (float)acc;
    return 3.01029995663981195f * __builtin_amdgcn_logf(precise_div(sig, fmaf(accf, rx.z, rx.w)));
}

}  // namespace d2d
