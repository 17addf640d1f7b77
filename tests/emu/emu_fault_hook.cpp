// emu_fault_hook.cpp -- the one-shot test hooks of the checked and sealed calls on the CPU (TEST INFRASTRUCTURE ONLY).
//
// Compiles fhe_reliability_gpu_amd/csrc/fault_hook.hpp -- the records the context stores, the setters' shared validation, take()
// and the check-record builder -- with g++, so that what the setters accept, refuse and store can be compared with the rules of
// include/fhe_mi355x.h without a GPU.  The library never links this file.
//
//   g++ -O2 -std=c++17 -shared -fPIC -I<csrc> emu_fault_hook.cpp -o libemu_fault_hook.so
#include "fault_hook.hpp"

using namespace fhe;

namespace {

const StagedRules *rules_of(int family)
{
    static const StagedRules *const r[4] = {&KSC_RULES, &RSC_RULES, &HRC_RULES, &BSGS_RULES};
    return family >= 0 && family < 4 ? r[family] : nullptr;
}

void put(long long out[6], const StagedFault &f)
{
    const long long v[6] = {f.block, f.stage, f.point, f.unit, f.coeff, f.bit};
    for (int i = 0; i < 6; i++) out[i] = v[i];
}

void put(long long out[5], const SealHook &f)
{
    const long long v[5] = {f.sel, f.idx, f.row, f.coeff, f.bit};
    for (int i = 0; i < 5; i++) out[i] = v[i];
}

void put(long long out[4], const PointFault &f)
{
    const long long v[4] = {f.point, (long long)f.unit, (long long)f.coeff, f.bit};
    for (int i = 0; i < 4; i++) out[i] = v[i];
}

} // namespace

extern "C" {

// number of stages of a family's hook (0 key switch, 1 rescale, 2 hoisted rotations, 3 BSGS product), -1 for another family
int emu_hook_stages(int family) { return rules_of(family) ? rules_of(family)->n_stages : -1; }

// A hook that holds `before` ({block, stage, point, unit, coeff, bit}) is armed with the setter's arguments: returns 1 where the
// setter accepts, 0 where it refuses, -1 for an unknown family; stored = the hook afterwards
int emu_hook_arm(int family, const long long before[6], int block, int stage, int point, int unit, long long coeff, int bit, long long stored[6])
{
    if (!rules_of(family)) return -1;
    StagedFault h{(int)before[0], (int)before[1], (int)before[2], (int)before[3], (int)before[5], before[4]};
    const bool ok = h.arm(*rules_of(family), block, stage, point, unit, coeff, bit);
    put(stored, h);
    return ok;
}

// the hook armed as above (returns the setter's answer), then taken twice: first / second = what the two calls got, stored = the hook afterwards
int emu_hook_take_twice(int family, int block, int stage, int point, int unit, long long coeff, int bit, long long first[6], long long second[6],
                        long long stored[6])
{
    if (!rules_of(family)) return -1;
    StagedFault h;
    const bool ok = h.arm(*rules_of(family), block, stage, point, unit, coeff, bit);
    put(first, h.take());
    put(second, h.take());
    put(stored, h);
    return ok;
}

// the same two steps for the hooks of one step; max_point = the setter's highest point
int emu_point_arm(int max_point, const long long before[4], int point, int unit, long long coeff, int bit, long long stored[4])
{
    PointHook h;
    static_cast<PointFault &>(h) = PointFault{(int)before[0], (u32)before[1], (u64)before[2], (int)before[3]};
    const bool ok = h.arm(max_point, point, unit, coeff, bit);
    put(stored, h);
    return ok;
}

int emu_point_take_twice(int max_point, int point, int unit, long long coeff, int bit, long long first[4], long long second[4], long long stored[4])
{
    PointHook h;
    const bool ok = h.arm(max_point, point, unit, coeff, bit);
    put(first, h.take());
    put(second, h.take());
    put(stored, h);
    return ok;
}

// the hooks of the sealed calls: a hook that holds `before` ({sel, idx, row, coeff, bit}) is armed with a setter's arguments as that
// setter passes them on (max_sel = its highest selector); returns 1 where the setter accepts, 0 where it refuses
int emu_seal_arm(int max_sel, const long long before[5], int sel, int idx, int row, long long coeff, int bit, long long stored[5])
{
    SealHook h{(int)before[0], (int)before[1], (int)before[2], (int)before[4], before[3]};
    const bool ok = h.arm(max_sel, sel, idx, row, coeff, bit);
    put(stored, h);
    return ok;
}

int emu_seal_take_twice(int max_sel, int sel, int idx, int row, long long coeff, int bit, long long first[5], long long second[5], long long stored[5])
{
    SealHook h;
    const bool ok = h.arm(max_sel, sel, idx, row, coeff, bit);
    put(first, h.take());
    put(second, h.take());
    put(stored, h);
    return ok;
}

// is the word of the armed hook {row, coeff} inside a call of `rows` rows of 2^log_n words
int emu_seal_inside(int row, long long coeff, unsigned long long rows, int log_n)
{
    const SealHook h{0, 0, row, 0, coeff};
    return h.inside((size_t)rows, log_n);
}

// bc_check of the record {block, stage, point, unit, coeff, bit} as seen from (at_block, at_stage), over the unit window [u0, u1)
// (windowed == 0: the default window).  out = {fault_point, fault_unit, fault_coeff}, *mask = fault_mask; returns 1 where the
// record carries the caller's flags pointer
int emu_bc_check(const long long rec[6], int at_block, int at_stage, int windowed, int u0, int u1, long long out[3], u64 *mask)
{
    const StagedFault f{(int)rec[0], (int)rec[1], (int)rec[2], (int)rec[3], (int)rec[5], rec[4]};
    u32 flags[1] = {0};
    const BcCheck k = windowed ? bc_check(f.at(at_block, at_stage), flags, u0, u1) : bc_check(f.at(at_block, at_stage), flags);
    out[0] = k.fault_point;
    out[1] = k.fault_unit;
    out[2] = (long long)k.fault_coeff;
    *mask = k.fault_mask;
    return k.flags == flags;
}

} // extern "C"
