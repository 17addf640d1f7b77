// scalar_checked.hip -- the word-wise scalar multiply / affine map c = a s_l + o_l mod q_l with every word checked against
// a s (+ o) = k q + c modulo 2^32 - 1 (scalar_check.hpp): the BGV steps of the checked key switch and mod switch, and
// fhe_scalar_affine_checked.  A translation unit of its own, so that every other kernel compiles exactly as before.  Streams from
// HBM like k_modadd_checked: one word per lane, the loop, grid and addressing of k_scalar_affine (a window of limbs of n_poly
// polynomials poly_stride rows apart, in place allowed: a lane reads and writes the same word), the word read once with a
// non-temporal load, the per-limb scalars passed by value and uniform per row; the residue work is 32-bit lane arithmetic and
// one FP64 estimate beside the 64-bit Barrett step; a failing lane ORs its unit's flag word with a global atomic, a clean run
// stores nothing extra.  No LDS.
#include "checked_kernel.hpp"
#include "scalar_check.hpp"

namespace fhe {

// PointwiseArgs as k_scalar_affine takes them (b unused); k.flags = [units] (poly * limbs + l), k.fault_unit indexes them
template <bool ADD, bool HOOK>
__global__ __launch_bounds__(256) void k_scalar_affine_checked(PointwiseArgs p, ScalarVec mul, ScalarVec add, BcCheck k)
{
    const u64 n = (u64)1 << p.logn;
    const u64 total = (u64)p.units << p.logn;
    for (u64 i_ = blockIdx.x * (u64)blockDim.x + threadIdx.x; i_ < total; i_ += (u64)gridDim.x * blockDim.x) {
        const u32 unit = (u32)(i_ >> p.logn);
        const u32 poly = unit / p.limbs, l = unit % p.limbs;
        const LimbParams &lp = p.lp[p.limb0 + l];
        const u64 q = lp.q;
        const u64 coeff = i_ & (n - 1);
        const u64 i = (((u64)poly * p.poly_stride + l) << p.logn) + coeff;
        u32 fl;
        p.c[i] = checked_scalar_affine<ADD>(__builtin_nontemporal_load(p.a + i), mul.v[l], ADD ? add.v[l] : 0, q, lp.barrett_lo, lp.barrett_hi, lp.ninv,
                                            res64(q), fl, fault_at<HOOK>(k, unit, coeff));
        if (fl) atomicOr(k.flags + unit, fl);
    }
}

hipError_t launch_scalar_affine_checked(hipStream_t st, const PointwiseArgs &p, const ScalarVec &mul, const ScalarVec *add, const BcCheck &k)
{
    const u64 total = (u64)p.units << p.logn;
    if (!total) return hipSuccess;
    const dim3 grid(checked_grid(total, 8192));
    if (add) return launch_checked(k_scalar_affine_checked<true, false>, k_scalar_affine_checked<true, true>, k, grid, st, p, mul, *add, k);
    return launch_checked(k_scalar_affine_checked<false, false>, k_scalar_affine_checked<false, true>, k, grid, st, p, mul, mul, k);
}

} // namespace fhe
