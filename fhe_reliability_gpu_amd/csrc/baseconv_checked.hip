// baseconv_checked.hip -- residue-checked RNS base conversions: fhe_baseconv_exact / fhe_baseconv_fast with every digit and
// every output word checked against its integer identity modulo 2^32 - 1 (baseconv_check.hpp).  A translation unit of its
// own, so that the base-conversion kernels of aux_kernels.hip compile exactly as before.  One lane = one coefficient, limb
// rows read and written at stride N as the unchecked kernels do; a failing lane ORs its unit's flag word with a global
// atomic, a clean run stores nothing extra.
#include "checked_kernel.hpp"
#include "baseconv_check.hpp"

namespace fhe {

constexpr int BCC_MAX_LIMBS = 64;

// the constants in LDS are invariant in the coefficient loop: without this the compiler hoists every read out of it
__device__ __forceinline__ void bcc_no_hoist() { __asm__ volatile("" ::: "memory"); }

// Exact conversion.  M > 0: the number of input limbs is a compile-time constant (bases of up to 16 limbs: every key-switch
// digit, every mod-down) -- digits and their residues in registers, straight-line code, the digit table and this workgroup's
// slice of the output table staged in LDS once per workgroup.  M = 0: any m up to 64, digits in a per-lane array, constants
// through scalar loads.  blockIdx.y selects a slice of `oc` outputs; every slice recomputes (and checks) the digits.
template <int M, bool HOOK>
__global__ __launch_bounds__(256) void k_bc_exact_checked(BcCheckedJob cj, u64 N, u32 oc)
{
    constexpr bool FIXED = M > 0;
    constexpr int MM = FIXED ? M : BCC_MAX_LIMBS, OCMAX = 64, UNR = FIXED ? M : 1;
    __shared__ Tw s_dig[FIXED ? M * M : 1], s_hor[FIXED ? OCMAX * M : 1];
    __shared__ u64 s_p[FIXED ? M : 1], s_q[FIXED ? OCMAX : 1];
    const BcJob &job = cj.job;
    const BaseConvPlanDev &pl = job.pl;
    const u64 *__restrict__ in = job.in;
    u64 *__restrict__ out = job.out;
    const int m = FIXED ? M : pl.m, k = pl.k;
    // the plan's tables are never written by a kernel: constant address space, so uniform reads become scalar loads
    const Tw FHE_CONSTANT *dig = (const Tw FHE_CONSTANT *)(__UINTPTR_TYPE__)cj.dig, *hor = (const Tw FHE_CONSTANT *)(__UINTPTR_TYPE__)cj.hor;
    const u64 FHE_CONSTANT *mod_in = (const u64 FHE_CONSTANT *)(__UINTPTR_TYPE__)pl.mod_in, *mod_out = (const u64 FHE_CONSTANT *)(__UINTPTR_TYPE__)pl.mod_out;
    const u32 FHE_CONSTANT *rows = (const u32 FHE_CONSTANT *)(__UINTPTR_TYPE__)job.in_rows;
    const int o0 = (int)blockIdx.y * (int)oc, o1 = o0 + (int)oc < k ? o0 + (int)oc : k, cnt = o1 - o0;
    if (cnt <= 0) return;
    if (FIXED) {
        for (int t = threadIdx.x; t < M * M; t += blockDim.x) s_dig[t] = dig[t];
        for (int t = threadIdx.x; t < cnt * M; t += blockDim.x) s_hor[t] = hor[(t % M) * k + o0 + t / M];       // [output][limb]
        for (int t = threadIdx.x; t < M; t += blockDim.x) s_p[t] = mod_in[t];
        for (int t = threadIdx.x; t < cnt; t += blockDim.x) s_q[t] = mod_out[o0 + t];
        __syncthreads();
    }
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < N; i += (u64)gridDim.x * blockDim.x) {
        bcc_no_hoist();
        u64 c[MM];
        u32 rc[MM];
#pragma unroll UNR
        for (int j = 0; j < MM; j++) {
            if (j < m) {
                const u64 p = FIXED ? s_p[j] : mod_in[j];
                const u64 row = rows ? (u64)rows[j] : (u64)j;
                u32 fl;
                c[j] = bc_checked_digit<UNR>(in[row * N + i], j, c, rc,
                                        [&](int l) -> Tw { if (FIXED) return s_dig[l * M + j]; const Tw t = dig[l * m + j]; return t; }, p, res64(p), fl,
                                        fault_at<HOOK>(cj.chk, (u32)j, i));
                rc[j] = res64(c[j]);
                if (fl) atomicOr(cj.chk.flags + j, fl);
            }
        }
        for (int o = o0; o < o1; o++) {
            bcc_no_hoist();
            const u64 q = FIXED ? s_q[o - o0] : mod_out[o];
            u32 fl;
            const u64 w = bc_checked_out<UNR>(m, c, rc, [&](int l) -> Tw { if (FIXED) return s_hor[(o - o0) * M + l]; const Tw t = hor[l * k + o]; return t; }, q,
                                         res64(q), fl, fault_at<HOOK>(cj.chk, (u32)(m + o), i));
            out[(u64)((u32)o < job.gap_at ? o : o + job.gap) * N + i] = w;
            if (fl) atomicOr(cj.chk.flags + m + o, fl);
        }
    }
}

// Fast conversion (k_bconv_fast): out[o] = sum_j (in_j C_jo mod q_o), not reduced.  The input words of a coefficient are
// re-read per output from the cache, as the unchecked kernel does.
template <bool HOOK>
__global__ __launch_bounds__(256) void k_bconv_fast_checked(u64 *__restrict__ out, const u64 *__restrict__ in, BaseConvPlanDev pl, BcCheck chk, u64 N)
{
    const u64 FHE_CONSTANT *mod_out = (const u64 FHE_CONSTANT *)(__UINTPTR_TYPE__)pl.mod_out;
    const u64 FHE_CONSTANT *coef = (const u64 FHE_CONSTANT *)(__UINTPTR_TYPE__)pl.fast_coef, *shoup = (const u64 FHE_CONSTANT *)(__UINTPTR_TYPE__)pl.fast_coef_shoup;
    const int m = pl.m, k = pl.k;
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < N; i += (u64)gridDim.x * blockDim.x) {
        for (int o = 0; o < k; o++) {
            const u64 q = mod_out[o];
            u32 fl;
            out[(u64)o * N + i] = bc_checked_fast(m, [&](int j) { return in[(u64)j * N + i]; }, [&](int j) { return Tw{coef[j * k + o], shoup[j * k + o]}; }, q,
                                                  res64(q), q * (u64)m, fl, fault_at<HOOK>(chk, (u32)o, i));
            if (fl) atomicOr(chk.flags + o, fl);
        }
    }
}

// aim at >= `target` workgroups: slice the k outputs over blockIdx.y while a slice stays at least as large as the digit
// computation it repeats (the rule of the unchecked launcher)
static u32 bcc_slices(u32 gx, int m, int k, u32 target)
{
    u32 slices = 1;
    while (gx * slices < target && slices * 2 <= (u32)k && (u32)k / (slices * 2) >= (u32)(m + 1) / 2) slices *= 2;
    return slices;
}

// the instantiation for a base of m limbs
using BcExactKernel = void (*)(BcCheckedJob, u64, u32);
template <bool HOOK>
static BcExactKernel bc_exact_kernel(int m)
{
    switch (m <= 16 ? m : 0) {
#define FHE_BCC(MM) case MM: return k_bc_exact_checked<MM, HOOK>;
        FHE_BCC(1) FHE_BCC(2) FHE_BCC(3) FHE_BCC(4) FHE_BCC(5) FHE_BCC(6) FHE_BCC(7) FHE_BCC(8)
        FHE_BCC(9) FHE_BCC(10) FHE_BCC(11) FHE_BCC(12) FHE_BCC(13) FHE_BCC(14) FHE_BCC(15) FHE_BCC(16)
#undef FHE_BCC
    default: return k_bc_exact_checked<0, HOOK>;
    }
}

hipError_t launch_baseconv_exact_checked(hipStream_t st, const BcCheckedJob &cj, u64 N)
{
    const BaseConvPlanDev &pl = cj.job.pl;
    if (pl.m < 1 || pl.k < 1 || pl.m > BCC_MAX_LIMBS || pl.k > 64) return hipErrorInvalidValue;
    if (!N) return hipSuccess;
    const u32 gx = checked_grid(N, 16384);
    const u32 slices = bcc_slices(gx, pl.m, pl.k, 1024), oc = ((u32)pl.k + slices - 1) / slices;
    const dim3 grid(gx, ((u32)pl.k + oc - 1) / oc);
    return launch_checked(bc_exact_kernel<false>(pl.m), bc_exact_kernel<true>(pl.m), cj.chk, grid, st, cj, N, oc);
}

hipError_t launch_bconv_fast_checked(hipStream_t st, u64 *out, const u64 *in, const BaseConvPlanDev &pl, const BcCheck &chk, u64 N)
{
    if (pl.m < 1 || pl.k < 1 || pl.m > BCC_MAX_LIMBS || pl.k > 64) return hipErrorInvalidValue;
    if (!N) return hipSuccess;
    return launch_checked(k_bconv_fast_checked<false>, k_bconv_fast_checked<true>, chk, dim3(checked_grid(N, 4096)), st, out, in, pl, chk, N);
}

} // namespace fhe
