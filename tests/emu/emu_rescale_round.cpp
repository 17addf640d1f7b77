// emu_rescale_round.cpp -- the per-word step of the round-to-nearest rescale (csrc/rescale_round.hpp) compiled for the CPU, as
// the kernels run it: the canonical residue, and that residue as an element of either arithmetic path, read back through the
// path's own canonical().  tests/test_emu_rescale_round.py holds all three against Python integers.
#include "rescale_round.hpp"

using namespace fhe;

extern "C" {

// out[i] = round_residue(y[i], q, (q - 1) / 2, qj)
void emu_round_residue(const u64 *y, size_t n, u64 q, u64 qj, u64 *out)
{
    const u64 h = (q - 1) / 2;
    for (size_t i = 0; i < n; i++) out[i] = round_residue(y[i], q, h, qj);
}

// the same taken into limb j's arithmetic as the kernels take it -- from_canonical of the word, what convert_in and the second
// input's apply() do -- and read back through the path's canonical(): path 0 = ArithF64 (qj < 2^50), 1 = ArithU64 (qj < 2^61)
int emu_round_residue_path(const u64 *y, size_t n, u64 q, u64 qj, int path, u64 *out)
{
    const u64 h = (q - 1) / 2;
    LimbParams p{};
    p.q = qj;
    p.two_q = 2 * qj;
    p.n = (double)qj;
    p.ninv = 1.0 / (double)qj;
    if (path == PATH_F64) {
        if (qj >> 50) return 1;
        const ArithF64::Ctx c = ArithF64::make_ctx(p);
        for (size_t i = 0; i < n; i++) out[i] = ArithF64::canonical(ArithF64::from_canonical(round_residue(y[i], q, h, c.q)), c);
    } else {
        if (qj >> 61) return 1;
        const ArithU64::Ctx c = ArithU64::make_ctx(p);
        for (size_t i = 0; i < n; i++) out[i] = ArithU64::canonical(ArithU64::from_canonical(round_residue(y[i], q, h, c.q)), c);
    }
    return 0;
}

} // extern "C"
