// bsgs_checked.hip -- the two kernels of the BSGS matrix-vector product that had no checked form: the inner sum over the baby
// steps (k_diag_mac) and the add that folds a giant rotation into the result (k_modadd), every word checked against its integer
// identity modulo 2^32 - 1 (bsgs_check.hpp).  A translation unit of its own, so that the kernels of aux_kernels.hip compile exactly
// as before.  Both stream from HBM, one element per lane, same loops, grids, loads and stores as the unchecked kernels; the residue
// work is 32-bit lane arithmetic beside the 64-bit products; a failing lane ORs its unit's flag word with a global atomic, a clean
// run stores nothing extra.  No LDS.
#include "checked_kernel.hpp"
#include "bsgs_check.hpp"

namespace fhe {

template <class D, bool HOOK>
__device__ __forceinline__ void diag_mac_elem_checked(const DiagMacArgs &a, const BcCheck &k, u64 e, const LimbParams &p)
{
    const u32 l = (u32)(e >> a.logn);
    const u64 i = e & (((u64)1 << a.logn) - 1);
    const PwFault f0 = fault_at<HOOK>(k, l, i), f1 = fault_at<HOOK>(k, a.limbs + l, i);
    DiagDot<D> s;
    for (u32 b = 0; b < a.n1; b++) {
        u64 d, y0, y1;
        diag_mac_load(a, b, e, d, y0, y1);
        s.mac(d, y0, y1, b, p, f0, f1);
    }
    u64 c0, c1;
    u32 fl0, fl1;
    s.finish(a.n1, p, c0, c1, fl0, fl1, f0, f1);
    a.out0[e] = c0;
    a.out1[e] = c1;
    if (fl0) atomicOr(k.flags + l, fl0);
    if (fl1) atomicOr(k.flags + a.limbs + l, fl1);
}

// DiagMacArgs as k_diag_mac takes them; k.flags = [2][limbs] (part, limb)
template <bool HOOK>
__global__ __launch_bounds__(256) void k_diag_mac_checked(DiagMacArgs a, BcCheck k)
{
    const u64 total = (u64)a.limbs << a.logn;
    for (u64 e = blockIdx.x * (u64)blockDim.x + threadIdx.x; e < total; e += (u64)gridDim.x * blockDim.x) {
        const LimbParams &p = a.lp[a.limb0 + (u32)(e >> a.logn)];
        if (p.path == PATH_F64) diag_mac_elem_checked<KsDotF64, HOOK>(a, k, e, p);
        else diag_mac_elem_checked<KsDotU64, HOOK>(a, k, e, p);
    }
}

// PointwiseArgs as k_modadd takes them; k.flags = [units] (poly * limbs + l), k.fault_unit indexes them
template <bool HOOK>
__global__ __launch_bounds__(256) void k_modadd_checked(PointwiseArgs p, BcCheck k)
{
    const u64 n = (u64)1 << p.logn;
    const u64 total = (u64)p.units << p.logn;
    for (u64 i_ = blockIdx.x * (u64)blockDim.x + threadIdx.x; i_ < total; i_ += (u64)gridDim.x * blockDim.x) {
        const u32 unit = (u32)(i_ >> p.logn);
        const u32 poly = unit / p.limbs, l = unit % p.limbs;
        const LimbParams &lp = p.lp[p.limb0 + l];
        const u64 q = lp.q;
        const u64 i = (((u64)poly * p.poly_stride + l) << p.logn) + (i_ & (n - 1));
        u32 fl;
        p.c[i] = checked_modadd(p.a[i], p.b[i], q, lp.barrett_lo, lp.barrett_hi, res64(q), fl, fault_at<HOOK>(k, unit, i_ & (n - 1)));
        if (fl) atomicOr(k.flags + unit, fl);
    }
}

hipError_t launch_diag_mac_checked(hipStream_t st, const DiagMacArgs &a, const BcCheck &k)
{
    const u64 total = (u64)a.limbs << a.logn;
    if (!total || !a.n1) return hipSuccess;
    return launch_checked(k_diag_mac_checked<false>, k_diag_mac_checked<true>, k, dim3(checked_grid(total, 16384)), st, a, k);
}

hipError_t launch_modadd_checked(hipStream_t st, const PointwiseArgs &p, const BcCheck &k)
{
    const u64 total = (u64)p.units << p.logn;
    if (!total) return hipSuccess;
    return launch_checked(k_modadd_checked<false>, k_modadd_checked<true>, k, dim3(checked_grid(total, 8192)), st, p, k);
}

} // namespace fhe
