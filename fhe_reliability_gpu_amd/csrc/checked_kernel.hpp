// checked_kernel.hpp -- what the residue-checked streaming kernels share (pointwise_checked.hip, baseconv_checked.hip,
// keyswitch_checked.hip, bsgs_checked.hip, rescale_checked.hip): how a lane finds out whether the one-shot test fault is its
// own, the 1-D grid, and the launch that picks the hooked or the clean instantiation.  The check record is BcCheck
// (fault_hook.hpp) for all of them.
#pragma once
#include "ntt_launch.hpp"
#include "residue_check.hpp"

namespace fhe {

// HOOK: the call's one-shot test fault (fhe_ctx_inject_fault_*) is armed -- a separate instantiation, so that the clean
// kernels carry no compare against the fault's unit and coefficient.  The fault is a function of (unit, coefficient) alone:
// every workgroup that recomputes a value (a base-conversion digit, for its slice of the outputs) sees the same wrong value.
template <bool HOOK>
__device__ __forceinline__ PwFault fault_at(const BcCheck &k, u32 unit, u64 coeff)
{
    if (!HOOK) return PwFault{-1, 0};
    return PwFault{k.fault_point, unit == k.fault_unit && coeff == k.fault_coeff ? k.fault_mask : 0};
}

// workgroups of 256 lanes for `total` lanes of a grid-stride loop: at least one, at most `cap`
inline u32 checked_grid(u64 total, u32 cap)
{
    const u64 want = (total + 255) / 256;
    return (u32)(want < 1 ? 1 : want > cap ? cap : want);
}

// launch `hooked` when a test fault is armed, `clean` otherwise: the same kernel at HOOK = true / false
template <class... P, class... A>
hipError_t launch_armed(void (*clean)(P...), void (*hooked)(P...), bool armed, dim3 grid, hipStream_t st, const A &...args)
{
    hipLaunchKernelGGL(armed ? hooked : clean, grid, dim3(256), 0, st, args...);
    return hipGetLastError();
}

// the same where k's fault is the only one the kernel knows
template <class... P, class... A>
hipError_t launch_checked(void (*clean)(P...), void (*hooked)(P...), const BcCheck &k, dim3 grid, hipStream_t st, const A &...args)
{
    return launch_armed(clean, hooked, k.fault_point >= 0, grid, st, args...);
}

} // namespace fhe
