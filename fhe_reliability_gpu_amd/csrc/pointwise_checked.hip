// pointwise_checked.hip -- residue-checked element-wise products: fhe_modmul / fhe_modmul_acc and fhe_tensor_product with
// every word checked against a b (+ o) = k q + c modulo 2^32 - 1 (residue_check.hpp).  A translation unit of its own, so
// that k_modmul and k_tensor (aux_kernels.hip) compile exactly as before.  Same loops, grids and non-temporal rule as the
// unchecked kernels; a failing lane ORs its unit's flag word with a global atomic, a clean run stores nothing extra.
#include "ntt_launch.hpp"
#include "residue_check.hpp"

namespace fhe {

// HOOK: the one-shot test fault of fhe_ctx_inject_fault_pointwise is armed (a separate instantiation, so that the clean
// kernels carry no compare against the fault index)
template <bool HOOK>
__device__ __forceinline__ PwFault pw_fault_at(const PwCheck &k, u64 elem)
{
    if (!HOOK) return PwFault{-1, 0};
    return PwFault{k.fault_point, elem == k.fault_idx ? k.fault_mask : 0};
}

template <bool ACC, bool NT, bool HOOK>
__global__ __launch_bounds__(256) void k_modmul_checked(PointwiseArgs p, PwCheck k)
{
    typedef u64 u64x2 __attribute__((ext_vector_type(2)));
    const u64 n = (u64)1 << p.logn;
    const u64 total = (u64)p.units << p.logn;
    for (u64 i_ = (blockIdx.x * (u64)blockDim.x + threadIdx.x) * 2; i_ < total; i_ += (u64)gridDim.x * blockDim.x * 2) {
        const u32 unit = (u32)(i_ >> p.logn);
        const u32 poly = unit / p.limbs, l = unit % p.limbs;
        const LimbParams &lp = p.lp[p.limb0 + l];
        const u64 q = lp.q, r0 = lp.barrett_lo, r1 = lp.barrett_hi;
        const u32 rq = res64(q);
        const u64 i = (((u64)poly * p.poly_stride + l) << p.logn) + (i_ & (n - 1));
        ulonglong2 a, b, o{0, 0};
        if (NT) {
            const u64x2 va = __builtin_nontemporal_load(reinterpret_cast<const u64x2 *>(p.a + i)), vb = __builtin_nontemporal_load(reinterpret_cast<const u64x2 *>(p.b + i));
            a = ulonglong2{va.x, va.y};
            b = ulonglong2{vb.x, vb.y};
        } else {
            a = *reinterpret_cast<const ulonglong2 *>(p.a + i);
            b = *reinterpret_cast<const ulonglong2 *>(p.b + i);
        }
        if (ACC) o = *reinterpret_cast<const ulonglong2 *>(p.c + i);
        u32 fx, fy;
        ulonglong2 c;
        c.x = checked_modmul_barrett<ACC>(a.x, b.x, o.x, q, r0, r1, rq, fx, pw_fault_at<HOOK>(k, i_));
        c.y = checked_modmul_barrett<ACC>(a.y, b.y, o.y, q, r0, r1, rq, fy, pw_fault_at<HOOK>(k, i_ + 1));
        if (NT) __builtin_nontemporal_store(u64x2{c.x, c.y}, reinterpret_cast<u64x2 *>(p.c + i));
        else *reinterpret_cast<ulonglong2 *>(p.c + i) = c;
        if (fx | fy) atomicOr(k.flags + unit, fx | fy);      // both elements of a lane lie in one unit (N >= 2)
    }
}

template <bool HOOK>
__global__ __launch_bounds__(256) void k_tensor_checked(TensorArgs t, PwCheck k)
{
    const u64 total = (u64)t.limbs << t.logn;
    for (u64 e = blockIdx.x * (u64)blockDim.x + threadIdx.x; e < total; e += (u64)gridDim.x * blockDim.x) {
        const u32 l = (u32)(e >> t.logn);
        const LimbParams &p = t.lp[t.limb0 + l];
        const u64 a0 = t.a0[e], a1 = t.a1[e], b0 = t.b0[e], b1 = t.b1[e];
        const u64 x0[1] = {a0}, y0[1] = {b0}, x2[1] = {a1}, y2[1] = {b1};
        const u64 x1[2] = {a0, a1}, y1[2] = {b1, b0};
        const PwFault none{-1, 0};
        u32 f0, f1, f2;
        if (p.path == PATH_F64) {
            t.d0[e] = checked_dot_f64<1>(x0, y0, p, f0, none);
            t.d1[e] = checked_dot_f64<2>(x1, y1, p, f1, pw_fault_at<HOOK>(k, e));
            t.d2[e] = checked_dot_f64<1>(x2, y2, p, f2, none);
        } else {
            t.d0[e] = checked_dot_u64<1>(x0, y0, p, f0, none);
            t.d1[e] = checked_dot_u64<2>(x1, y1, p, f1, pw_fault_at<HOOK>(k, e));
            t.d2[e] = checked_dot_u64<1>(x2, y2, p, f2, none);
        }
        if (f0 | f1 | f2) {
            u32 *fl = k.flags + 3 * (u64)l;
            if (f0) atomicOr(fl, f0);
            if (f1) atomicOr(fl + 1, f1);
            if (f2) atomicOr(fl + 2, f2);
        }
    }
}

hipError_t launch_modmul_checked(hipStream_t st, const PointwiseArgs &p, bool accumulate, const PwCheck &k)
{
    const u64 total = (u64)p.units << p.logn;
    if (!total) return hipSuccess;
    u64 want = (total / 2 + 255) / 256;
    const u32 blocks = (u32)(want < 1 ? 1 : want > 8192 ? 8192 : want);
    const bool nt = total * 24 > ((u64)192 << 20);      // three buffers of the batch's size (launch_modmul's rule)
    const dim3 g(blocks), b(256);
    if (k.fault_point >= 0) {
        if (accumulate) hipLaunchKernelGGL((k_modmul_checked<true, false, true>), g, b, 0, st, p, k);
        else hipLaunchKernelGGL((k_modmul_checked<false, false, true>), g, b, 0, st, p, k);
    } else if (accumulate) hipLaunchKernelGGL((k_modmul_checked<true, false, false>), g, b, 0, st, p, k);
    else if (nt) hipLaunchKernelGGL((k_modmul_checked<false, true, false>), g, b, 0, st, p, k);
    else hipLaunchKernelGGL((k_modmul_checked<false, false, false>), g, b, 0, st, p, k);
    return hipGetLastError();
}

hipError_t launch_tensor_checked(hipStream_t st, const TensorArgs &p, const PwCheck &k)
{
    const u64 total = (u64)p.limbs << p.logn;
    if (!total) return hipSuccess;
    const u64 want = (total + 255) / 256;
    const dim3 g((u32)(want > 16384 ? 16384 : want)), b(256);
    if (k.fault_point >= 0) hipLaunchKernelGGL(k_tensor_checked<true>, g, b, 0, st, p, k);
    else hipLaunchKernelGGL(k_tensor_checked<false>, g, b, 0, st, p, k);
    return hipGetLastError();
}

} // namespace fhe
