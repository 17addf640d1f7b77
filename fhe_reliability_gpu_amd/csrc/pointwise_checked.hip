// pointwise_checked.hip -- residue-checked element-wise products: fhe_modmul / fhe_modmul_acc and fhe_tensor_product with
// every word checked against a b (+ o) = k q + c modulo 2^32 - 1 (residue_check.hpp).  A translation unit of its own, so
// that k_modmul and k_tensor (aux_kernels.hip) compile exactly as before.  Same loops, grids and non-temporal rule as the
// unchecked kernels; a failing lane ORs its unit's flag word with a global atomic, a clean run stores nothing extra.
#include "checked_kernel.hpp"

namespace fhe {

template <bool ACC, bool NT, bool HOOK>
__global__ __launch_bounds__(256) void k_modmul_checked(PointwiseArgs p, BcCheck k)
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
        const u64 coeff = i_ & (n - 1);
        const u64 i = (((u64)poly * p.poly_stride + l) << p.logn) + coeff;
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
        c.x = checked_modmul_barrett<ACC>(a.x, b.x, o.x, q, r0, r1, rq, fx, fault_at<HOOK>(k, unit, coeff));
        c.y = checked_modmul_barrett<ACC>(a.y, b.y, o.y, q, r0, r1, rq, fy, fault_at<HOOK>(k, unit, coeff + 1));
        if (NT) __builtin_nontemporal_store(u64x2{c.x, c.y}, reinterpret_cast<u64x2 *>(p.c + i));
        else *reinterpret_cast<ulonglong2 *>(p.c + i) = c;
        if (fx | fy) atomicOr(k.flags + unit, fx | fy);      // both elements of a lane lie in one unit (N >= 2)
    }
}

template <bool HOOK>
__global__ __launch_bounds__(256) void k_tensor_checked(TensorArgs t, BcCheck k)
{
    const u64 total = (u64)t.limbs << t.logn;
    for (u64 e = blockIdx.x * (u64)blockDim.x + threadIdx.x; e < total; e += (u64)gridDim.x * blockDim.x) {
        const u32 l = (u32)(e >> t.logn);
        const LimbParams &p = t.lp[t.limb0 + l];
        const u64 a0 = t.a0[e], a1 = t.a1[e], b0 = t.b0[e], b1 = t.b1[e];
        const u64 x0[1] = {a0}, y0[1] = {b0}, x2[1] = {a1}, y2[1] = {b1};
        const u64 x1[2] = {a0, a1}, y1[2] = {b1, b0};
        const PwFault none{-1, 0}, f = fault_at<HOOK>(k, l, e & (((u64)1 << t.logn) - 1));      // f: of the d1 sum
        u32 f0, f1, f2;
        if (p.path == PATH_F64) {
            t.d0[e] = checked_dot_f64<1>(x0, y0, p, f0, none);
            t.d1[e] = checked_dot_f64<2>(x1, y1, p, f1, f);
            t.d2[e] = checked_dot_f64<1>(x2, y2, p, f2, none);
        } else {
            t.d0[e] = checked_dot_u64<1>(x0, y0, p, f0, none);
            t.d1[e] = checked_dot_u64<2>(x1, y1, p, f1, f);
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

hipError_t launch_modmul_checked(hipStream_t st, const PointwiseArgs &p, bool accumulate, const BcCheck &k)
{
    const u64 total = (u64)p.units << p.logn;
    if (!total) return hipSuccess;
    const bool nt = total * 24 > ((u64)192 << 20);      // three buffers of the batch's size (launch_modmul's rule)
    // the hooked form is never non-temporal
    const auto clean = accumulate ? k_modmul_checked<true, false, false> : nt ? k_modmul_checked<false, true, false> : k_modmul_checked<false, false, false>;
    const auto hooked = accumulate ? k_modmul_checked<true, false, true> : k_modmul_checked<false, false, true>;
    return launch_checked(clean, hooked, k, dim3(checked_grid(total / 2, 8192)), st, p, k);      // two elements per lane
}

hipError_t launch_tensor_checked(hipStream_t st, const TensorArgs &p, const BcCheck &k)
{
    const u64 total = (u64)p.limbs << p.logn;
    if (!total) return hipSuccess;
    return launch_checked(k_tensor_checked<false>, k_tensor_checked<true>, k, dim3(checked_grid(total, 16384)), st, p, k);
}

} // namespace fhe
