// keyswitch_checked.hip -- the two key-switch stages that had no checked form: the inner product with the key (k_ks_mac) and
// the mod-down tail (k_sub_scale), every word checked against its integer identity modulo 2^32 - 1 (keyswitch_check.hpp).  A
// translation unit of its own, so that the kernels of aux_kernels.hip compile exactly as before.  Both stream from HBM, one
// element per lane, same loops and grids as the unchecked kernels; the residue work is 32-bit lane arithmetic beside the 64-bit
// products; a failing lane ORs its unit's flag word with a global atomic, a clean run stores nothing extra.  No LDS.
#include "checked_kernel.hpp"
#include "keyswitch_check.hpp"

namespace fhe {

// the key is read once: non-temporal, so that it does not push the digits (read by both halves' neighbours) out of the caches
__device__ __forceinline__ u64 ks_load_key(const u64 *p) { return __builtin_nontemporal_load(p); }

template <class D, bool HOOK>
__device__ __forceinline__ void ks_mac_limb_checked(const KsMacArgs &a, const BcCheck &k, u32 j, u64 i, const LimbParams &p)
{
    const u64 N = (u64)1 << a.logn;
    D s0, s1;
    const PwFault f0 = fault_at<HOOK>(k, j, i), f1 = fault_at<HOOK>(k, a.M + j, i);
    const u32 tl = ks_mac_table_limb(a, j);
    for (u32 d = 0; d < a.dnum; d++) {
        u64 x;
        const u64 *key = ks_mac_load(a, tl, d, j, i, x);
        s0.mac(x, ks_load_key(key), d, p, f0);
        s1.mac(x, ks_load_key(key + (u64)a.M * N), d, p, f1);
    }
    u32 fl0, fl1;
    a.acc[(u64)j * N + i] = s0.finish(a.dnum, p, fl0, f0);
    a.acc[((u64)a.M + j) * N + i] = s1.finish(a.dnum, p, fl1, f1);
    if (fl0) atomicOr(k.flags + j, fl0);
    if (fl1) atomicOr(k.flags + a.M + j, fl1);
}

// KsMacArgs as k_ks_mac takes them; k.flags = [2][M] (half, row)
template <bool HOOK>
__global__ __launch_bounds__(256) void k_ks_mac_checked(KsMacArgs a, BcCheck k)
{
    const u64 total = (u64)a.M << a.logn;
    for (u64 e = blockIdx.x * (u64)blockDim.x + threadIdx.x; e < total; e += (u64)gridDim.x * blockDim.x) {
        const u32 j = (u32)(e >> a.logn);
        const u64 i = e & (((u64)1 << a.logn) - 1);
        const LimbParams &p = a.lp[j < a.cn ? a.clo + j : j + a.sp_shift];
        if (p.path == PATH_F64) ks_mac_limb_checked<KsDotF64, HOOK>(a, k, j, i, p);
        else ks_mac_limb_checked<KsDotU64, HOOK>(a, k, j, i, p);
    }
}

// SubScaleArgs as k_sub_scale takes them (blockIdx.y = half); k.flags = [halves][limbs]
template <bool HOOK>
__global__ __launch_bounds__(256) void k_sub_scale_checked(SubScaleArgs p, BcCheck k)
{
    const u32 h = blockIdx.y;
    u64 *out = h ? p.out1 : p.out0;
    const u64 *a = p.a ? p.a + (u64)h * p.a_stride : nullptr, *b = p.b ? p.b + (u64)h * p.b_stride : nullptr, *add = h ? p.add1 : p.add0;
    const u64 total = (u64)p.limbs << p.logn;
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < total; i += (u64)gridDim.x * blockDim.x) {
        const u32 l = (u32)(i >> p.logn);
        const LimbParams &lp = p.lp[p.limb0 + l];
        const u64 q = lp.q;
        u32 fl;
        out[i] = checked_sub_scale(a ? a[i] : 0, a != nullptr, b ? b[i] : 0, b != nullptr, p.scal[l], add ? add[i] : 0, add != nullptr, q, lp.barrett_lo,
                                   lp.barrett_hi, res64(q), fl, fault_at<HOOK>(k, h * p.limbs + l, i & (((u64)1 << p.logn) - 1)));
        if (fl) atomicOr(k.flags + h * p.limbs + l, fl);
    }
}

// dst[map[i]] = src[i]: the digit extensions' flags from the order of their conversion jobs (digit units, then output units)
// into the [dnum][M] limb order of the key switch's flag layout
__global__ void k_ks_flags_scatter(u32 *dst, const u32 *src, const u32 *map, u32 n)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const u32 v = src[i];
        if (v) dst[map[i]] = v;
    }
}

hipError_t launch_ks_mac_checked(hipStream_t st, const KsMacArgs &a, const BcCheck &k)
{
    const u64 total = (u64)a.M << a.logn;
    if (!total) return hipSuccess;
    return launch_checked(k_ks_mac_checked<false>, k_ks_mac_checked<true>, k, dim3(checked_grid(total, 16384)), st, a, k);
}

hipError_t launch_sub_scale_checked(hipStream_t st, const SubScaleArgs &p, const BcCheck &k)
{
    const u64 total = (u64)p.limbs << p.logn;
    if (!total) return hipSuccess;
    return launch_checked(k_sub_scale_checked<false>, k_sub_scale_checked<true>, k, dim3(checked_grid(total, 8192), p.out1 ? 2 : 1), st, p, k);
}

hipError_t launch_ks_flags_scatter(hipStream_t st, u32 *dst, const u32 *src, const u32 *map, u32 n)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_ks_flags_scatter, dim3((n + 255) / 256), dim3(256), 0, st, dst, src, map, n);
    return hipGetLastError();
}

} // namespace fhe
