// emu_seal_repair.cpp -- CPU emulation of the seal repair (TEST INFRASTRUCTURE ONLY).
//
// Compiles the repair functions of fhe_reliability_gpu_amd/csrc/seal_check.hpp -- the functions the kernels of seal_repair.hip call
// -- with g++ and runs k_row_repair's steps over one row on the host: a sweep that forms the three sums afresh and counts the words
// out of the window, the one-lane decision, the store, and the confirming sweep.  The two-sum locator a seal alone would allow is
// exported next to it, so that the tests can show which cases it would have accepted.  The library never links this file.
//
//   g++ -O2 -std=c++17 -shared -fPIC -I<csrc> emu_seal_repair.cpp -o libemu_seal_repair.so
#include "seal_check.hpp"

using namespace fhe;

namespace {

struct Sweep {
    u64 got[3];
    u32 n_out, out_idx;
};

Sweep sweep(const u64 *x, u32 n, u64 q)
{
    SealAcc3 a;
    Sweep s{{0, 0, 0}, 0, 0};
    for (u32 j = 0; j < n; j++) {
        a.add(x[j], j);
        if (x[j] >= q) s.n_out++, s.out_idx = j;
    }
    s.got[0] = seal_canonical(a.s0), s.got[1] = seal_canonical(a.s1), s.got[2] = seal_canonical(a.s2);
    return s;
}

} // namespace

extern "C" {

u64 emu_seal_mulmod(u64 a, u64 b) { return seal_mulmod(a, b); }
u64 emu_seal_inv(u64 a) { return seal_inv(a); }
u64 emu_seal_restore(u64 x_now, u64 d0) { return seal_restore(x_now, d0); }
long long emu_seal_locate(u64 d0, u64 d1, u64 d2, u32 n) { return seal_locate(d0, d1, d2, n); }

// sums[r] = {S0, S1, S2} of row r of x = [rows][n]
void emu_seal3(const u64 *x, size_t rows, u32 n, u64 *sums)
{
    for (size_t r = 0; r < rows; r++) {
        const Sweep s = sweep(x + r * n, n, ~(u64)0);
        for (int i = 0; i < 3; i++) sums[3 * r + i] = s.got[i];
    }
}

// S2 alone, the way k_row_locator accumulates it
u64 emu_seal_locator(const u64 *x, u32 n)
{
    u64 s2 = 0;
    for (u32 j = 0; j < n; j++) s2 = seal_fold(s2 + seal_w2mul(seal_fold(x[j]), j + 1));
    return seal_canonical(s2);
}

// what a locator made of S0 and S1 alone would do: the index D1 / D0 where it is integral and in range, else -1
long long emu_two_sum_locate(u64 d0, u64 d1, u32 n)
{
    if (d0 == 0) return -1;
    const u64 w = seal_mulmod(d1, seal_inv(d0));
    return w >= 1 && w <= n ? (long long)w - 1 : -1;
}

// k_row_repair on one flagged row x[n] (written where repaired) against stored = {S0, S1, S2}: report = {status, index, before, after}
void emu_seal_repair_row(u64 *x, u32 n, u64 q, const u64 *stored, u64 *report)
{
    const Sweep s = sweep(x, n, q);
    const SealVerdict v = seal_decide(s.got, stored, s.n_out, s.out_idx, n);
    int status = v.status;
    u64 index = 0, before = 0, after = 0;
    if (status == SEAL_REPAIRED) {
        index = v.index;
        before = x[index];
        if (seal_repair_word(before, v.d0, q, after)) {
            x[index] = after;
            const Sweep c = sweep(x, n, q);
            if (c.got[0] != stored[0] || c.got[1] != stored[1] || c.got[2] != stored[2] || c.n_out != 0) {
                x[index] = before;
                status = SEAL_UNCORRECTABLE;
            }
        } else {
            status = SEAL_UNCORRECTABLE;
        }
        if (status != SEAL_REPAIRED) index = 0, before = 0, after = 0;
    }
    report[0] = (u64)status, report[1] = index, report[2] = before, report[3] = after;
}

} // extern "C"
