// rescale_checked.hip -- the one rescale stage that had no checked form: the residues of the dropped limb modulo every remaining
// prime, every word checked against x = k q_j + delta_j modulo 2^32 - 1 (rescale_check.hpp).  A translation unit of its own, so
// that every other kernel compiles exactly as before.  Streams from HBM like k_ks_mac_checked: one lane per (part, coefficient)
// loads x once and stores its R residues (consecutive lanes, consecutive words of each limb), the residue work is 32-bit lane
// arithmetic beside the 64-bit Barrett step, the limb constants are uniform across the wavefront; a failing lane ORs its unit's
// flag word with a global atomic, a clean run stores nothing extra.  No LDS.
#include "checked_kernel.hpp"
#include "rescale_check.hpp"

namespace fhe {

// k.flags = [n_parts][R] (part, limb)
template <bool HOOK>
__global__ __launch_bounds__(256) void k_rescale_reduce_checked(RescaleReduceArgs a, BcCheck k)
{
    const u64 total = (u64)a.n_parts << a.logn;
    const u64 qlast = a.lp[a.R].q;
    for (u64 e = blockIdx.x * (u64)blockDim.x + threadIdx.x; e < total; e += (u64)gridDim.x * blockDim.x) {
        const u32 part = (u32)(e >> a.logn);
        const u64 i = e & (((u64)1 << a.logn) - 1);
        const u64 x = __builtin_nontemporal_load(a.x + e);      // read once
        const u32 rx = res64(x);
        u64 *out = a.delta + (((u64)part * a.R) << a.logn) + i;
        for (u32 j = 0; j < a.R; j++) {
            const LimbParams &p = a.lp[j];
            u32 fl;
            out[(u64)j << a.logn] = checked_reduce_word(x, qlast, p.q, p.barrett_lo, p.barrett_hi, rx, res64(p.q), fl, fault_at<HOOK>(k, part * a.R + j, i));
            if (fl) atomicOr(k.flags + part * a.R + j, fl);
        }
    }
}

hipError_t launch_rescale_reduce_checked(hipStream_t st, const RescaleReduceArgs &a, const BcCheck &k)
{
    const u64 total = (u64)a.n_parts << a.logn;
    if (!total || !a.R) return hipSuccess;
    return launch_checked(k_rescale_reduce_checked<false>, k_rescale_reduce_checked<true>, k, dim3(checked_grid(total, 16384)), st, a, k);
}

} // namespace fhe
