// fault_hook.hpp -- the one-shot test hooks of the checked and sealed calls (fhe_ctx_inject_fault_*): how a hook is stored in the context,
// armed by its setter, taken by the call it belongs to, and turned into the check record a launch reads.  Host only and free of
// HIP, so that tests/emu/emu_fault_hook.cpp compiles it with g++.
//
// A hook is armed by its setter, which validates what does not depend on a call, and is taken -- read and disarmed in one step,
// take() -- by the next checked call that runs the hook's step, whatever that call's outcome.  take() is the only place that
// disarms a hook.  What depends on the call (units, coefficients, points that exist only on some units) is checked by the call
// against the record it took, before anything is launched.
#pragma once
#include <climits>
#include <cstddef>

#include "galois_check.hpp"

namespace fhe {

// the check record of the residue-checked launches (ntt_launch.hpp): flags = the launch's flag words; fault_point >= 0: XOR
// fault_mask at that injection point (residue_check.hpp PW_AT_*) of unit fault_unit (index into flags), coefficient fault_coeff
struct BcCheck {
    u32 *flags;
    int fault_point;
    u32 fault_unit;
    u64 fault_coeff, fault_mask;
};

// ---- hooks of one step (pointwise, polynomial product, base conversion, Galois permutation): point < 0 = disarmed.  The
// pointwise and product hooks address an element of the call's window: unit stays 0, coeff is the element
using PointFault = GaloisFault;
struct PointHook : PointFault {
    PointFault take()
    {
        const PointFault f = *this;
        point = -1;
        return f;
    }
    // the setter's core: a negative point disarms; false (nothing stored) for what no call could honour
    bool arm(int max_point, int pt, int u, long long c, int b)
    {
        if (pt < 0) {
            take();
            return true;
        }
        if (pt > max_point || u < 0 || c < 0 || b < 0 || b > 63) return false;
        static_cast<PointFault &>(*this) = PointFault{pt, (u32)u, (u64)c, b};
        return true;
    }
};

// ---- hooks of the sealed calls, which flip one bit of word coeff of a row on the load that digests it: sel < 0 = disarmed.  sel is
// the setter's disarming argument, idx and row are its further indices (fhe_ctx lists the fields per setter)
struct SealHook {
    int sel = -1, idx = 0, row = 0, bit = 0;
    long long coeff = 0;

    SealHook take()
    {
        const SealHook f = *this;
        sel = -1;
        return f;
    }
    // the setter's core: a negative selector disarms; false (nothing stored) for what no call could honour
    bool arm(int max_sel, int s, int i, int r, long long c, int b)
    {
        if (s < 0) {
            take();
            return true;
        }
        if (s > max_sel || i < 0 || r < 0 || c < 0 || b < 0 || b > 63) return false;
        *this = SealHook{s, i, r, b, c};
        return true;
    }
    // does an armed hook's word lie inside a call of `rows` rows of 2^log_n words
    bool inside(size_t rows, int log_n) const { return (size_t)row < rows && !((u64)coeff >> log_n); }
};

// ---- hooks of a composite call, which address one of its stages: stage < 0 = disarmed
// per stage the highest injection point, or HOOK_TRANSFORM: a transform stage, whose one point lies between its two launches
// (the setter ignores `point` and stores 0)
// HOOK_NONE: a stage number the call does not have
constexpr int HOOK_TRANSFORM = -1, HOOK_NONE = -2;
struct StagedRules {
    int n_stages;
    int max_point[11];
};
constexpr StagedRules KSC_RULES{8, {HOOK_TRANSFORM, 3, HOOK_TRANSFORM, 3, HOOK_TRANSFORM, 3, HOOK_TRANSFORM, 3}};                   // key switch
constexpr StagedRules RSC_RULES{4, {HOOK_TRANSFORM, 3, HOOK_TRANSFORM, 3}};                                                         // rescale
constexpr StagedRules HRC_RULES{9, {HOOK_TRANSFORM, 3, HOOK_TRANSFORM, 3, HOOK_TRANSFORM, 3, HOOK_TRANSFORM, 3, GAL_AT_INDEX}};     // hoisted rotations
constexpr StagedRules BSGS_RULES{2, {3, 3}};                                                                                        // BSGS product
// BGV key switch: the key switch's stages plus 9 and 10, the two scalar stages (8 stays the hoisted rotations' permutation number);
// BGV mod switch: the rescale's plus 4 and 5.  Point 3 of a scalar stage passes the setter and is refused by the call (no addend)
constexpr StagedRules BGV_KSC_RULES{11, {HOOK_TRANSFORM, 3, HOOK_TRANSFORM, 3, HOOK_TRANSFORM, 3, HOOK_TRANSFORM, 3, HOOK_NONE, 3, 3}};
constexpr StagedRules BGV_RSC_RULES{6, {HOOK_TRANSFORM, 3, HOOK_TRANSFORM, 3, 3, 3}};

struct StagedFault {
    int block = 0;       // the rotation (hoisted rotations) or giant step (BSGS) the stage belongs to; 0 where there is none
    int stage = -1, point = 0, unit = 0, bit = 0;
    long long coeff = 0;

    StagedFault take()
    {
        const StagedFault f = *this;
        stage = -1;
        return f;
    }
    // the setter's core: a negative stage disarms; false (nothing stored) for what no call could honour
    bool arm(const StagedRules &r, int blk, int st, int pt, int u, long long c, int b)
    {
        if (st < 0) {
            take();
            return true;
        }
        if (st >= r.n_stages || r.max_point[st] == HOOK_NONE || blk < 0 || u < 0 || c < 0 || b < 0 || b > 63) return false;
        const bool transform = r.max_point[st] == HOOK_TRANSFORM;
        if (!transform && (pt < 0 || pt > r.max_point[st])) return false;
        *this = StagedFault{blk, st, transform ? 0 : pt, u, b, c};
        return true;
    }
    // this record where it addresses (blk, st), a disarmed one elsewhere
    StagedFault at(int blk, int st) const { return stage == st && block == blk ? *this : StagedFault{}; }
};

// the check record of one launch whose flag words are units [u0, u1) of the fault's stage: armed when f is armed and its unit lies
// in that window (the unit is rebased to the launch's flags)
inline BcCheck bc_check(const StagedFault &f, u32 *flags, int u0 = 0, int u1 = INT_MAX)
{
    if (f.stage < 0 || f.unit < u0 || f.unit >= u1) return BcCheck{flags, -1, 0, 0, 0};
    return BcCheck{flags, f.point, (u32)(f.unit - u0), (u64)f.coeff, (u64)1 << f.bit};
}

} // namespace fhe
