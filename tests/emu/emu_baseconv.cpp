// emu_baseconv.cpp -- CPU emulation of the residue-checked base conversions (TEST INFRASTRUCTURE ONLY).
//
// Compiles fhe_reliability_gpu_amd/csrc/baseconv_check.hpp -- the element functions the kernels of baseconv_checked.hip
// call -- with g++ and runs them over arrays of coefficients, with an optional bit flip at one injection point of one unit
// of every coefficient, so that digits, words and flag bits can be checked against Python integers without a GPU.  The
// constants are built here the way fhe_baseconv_create builds them.  The library never links this file.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -I<csrc> emu_baseconv.cpp -o libemu_baseconv.so
#include "baseconv_check.hpp"

#include <vector>

using namespace fhe;

namespace {

u64 mul_mod(u64 a, u64 b, u64 q) { return (u64)((unsigned __int128)a * b % q); }
u64 pow_mod(u64 a, u64 e, u64 q)
{
    u64 r = 1 % q;
    for (a %= q; e; e >>= 1, a = mul_mod(a, a, q))
        if (e & 1) r = mul_mod(r, a, q);
    return r;
}
u64 inv_mod(u64 a, u64 q) { return pow_mod(a, q - 2, q); }       // the moduli of the tests are primes
Tw shoup(u64 w, u64 q) { return Tw{w, (u64)(((unsigned __int128)w << 64) / q)}; }

// capi_baseconv.cpp fhe_baseconv_create: dig[l*m+j] = D_lj (l < j), dig[j*m+j] = A_j; hor[l*k+o] = E_lo; fast[j*k+o] = C_jo
struct Plan {
    int m, k;
    std::vector<u64> p, q;
    std::vector<Tw> dig, hor, fast;
    Plan(const u64 *mi, int m_, const u64 *mo, int k_) : m(m_), k(k_), p(mi, mi + m_), q(mo, mo + k_), dig((size_t)m_ * m_, Tw{0, 0}), hor((size_t)m_ * k_), fast((size_t)m_ * k_)
    {
        for (int j = 0; j < m; j++) {
            u64 prod = 1 % p[j];
            for (int l = j - 1; l >= 0; l--) {
                prod = mul_mod(prod, p[l] % p[j], p[j]);
                const u64 inv = inv_mod(prod, p[j]);
                dig[(size_t)l * m + j] = shoup(inv, p[j]);
                if (l == 0) dig[(size_t)j * m + j] = shoup(inv, p[j]);
            }
            if (j == 0) dig[0] = shoup(1 % p[0], p[0]);
        }
        for (int o = 0; o < k; o++) {
            u64 prod = 1 % q[o];
            for (int l = 0; l < m; l++) {
                hor[(size_t)l * k + o] = shoup(prod, q[o]);
                prod = mul_mod(prod, p[l] % q[o], q[o]);
            }
        }
        for (int j = 0; j < m; j++) {
            u64 hat = 1 % p[j];
            for (int l = 0; l < m; l++)
                if (l != j) hat = mul_mod(hat, p[l] % p[j], p[j]);
            const u64 inv = inv_mod(hat, p[j]);
            for (int o = 0; o < k; o++) {
                u64 hq = 1 % q[o];
                for (int l = 0; l < m; l++)
                    if (l != j) hq = mul_mod(hq, p[l] % q[o], q[o]);
                fast[(size_t)j * k + o] = shoup(mul_mod(hq, inv % q[o], q[o]), q[o]);
            }
        }
    }
};

PwFault fault_at(int point, int unit, int bit, int at) { return PwFault{point, point >= 0 && unit == at ? (u64)1 << bit : 0}; }

// aux_kernels.hip mulmod_shoup
u64 mulmod_shoup(u64 a, u64 w, u64 ws, u64 q)
{
    const u64 r = a * w - mulhi64(a, ws) * q;
    return r >= q ? r - q : r;
}

} // namespace

extern "C" {

// exact conversion of n coefficients, in = [m][n]; the fault (point >= 0) hits unit `unit` (digit j < m, output m + o) of
// every coefficient.  digits = [m][n], words = [k][n], flags = [m + k][n].  -2: the point does not exist on that unit.
int emu_bc_exact_checked(const u64 *mi, int m, const u64 *mo, int k, const u64 *in, size_t n, int point, int unit, int bit, u64 *digits,
                         u64 *words, u32 *flags)
{
    if (m < 1 || k < 1 || m > 64 || k > 64) return -1;
    if (point >= 0 && (unit < 0 || unit >= m + k || !bc_point_exists(point, unit < m ? unit + 1 : m))) return -2;
    const Plan pl(mi, m, mo, k);
    for (size_t i = 0; i < n; i++) {
        u64 c[64];
        u32 rc[64];
        for (int j = 0; j < m; j++) {
            c[j] = bc_checked_digit(in[(size_t)j * n + i], j, c, rc, [&](int l) { return pl.dig[(size_t)l * m + j]; }, pl.p[j], res64(pl.p[j]),
                                    flags[(size_t)j * n + i], fault_at(point, unit, bit, j));
            rc[j] = res64(c[j]);
            digits[(size_t)j * n + i] = c[j];
        }
        for (int o = 0; o < k; o++)
            words[(size_t)o * n + i] = bc_checked_out(m, c, rc, [&](int l) { return pl.hor[(size_t)l * k + o]; }, pl.q[o], res64(pl.q[o]),
                                                      flags[(size_t)(m + o) * n + i], fault_at(point, unit, bit, m + o));
    }
    return 0;
}

// the unchecked integer path (aux_kernels.hip bc_exact_body with BcU64): Shoup products, modular add / sub
int emu_bc_exact_plain(const u64 *mi, int m, const u64 *mo, int k, const u64 *in, size_t n, u64 *words)
{
    if (m < 1 || k < 1 || m > 64 || k > 64) return -1;
    const Plan pl(mi, m, mo, k);
    for (size_t i = 0; i < n; i++) {
        u64 c[64];
        for (int j = 0; j < m; j++) {
            const u64 p = pl.p[j];
            u64 t = mulmod_shoup(in[(size_t)j * n + i], pl.dig[(size_t)j * m + j].a, pl.dig[(size_t)j * m + j].b, p);
            for (int l = 0; l < j; l++) {
                const u64 b = mulmod_shoup(c[l], pl.dig[(size_t)l * m + j].a, pl.dig[(size_t)l * m + j].b, p);
                t = t >= b ? t - b : t + p - b;
            }
            c[j] = t;
        }
        for (int o = 0; o < k; o++) {
            const u64 q = pl.q[o];
            u64 acc = mulmod_shoup(c[0], pl.hor[o].a, pl.hor[o].b, q);
            for (int l = 1; l < m; l++) {
                const u64 s = acc + mulmod_shoup(c[l], pl.hor[(size_t)l * k + o].a, pl.hor[(size_t)l * k + o].b, q);
                acc = s >= q ? s - q : s;
            }
            words[(size_t)o * n + i] = acc;
        }
    }
    return 0;
}

// fast conversion; the fault hits output unit `unit` of every coefficient.  words = [k][n], flags = [k][n]
int emu_bc_fast_checked(const u64 *mi, int m, const u64 *mo, int k, const u64 *in, size_t n, int point, int unit, int bit, u64 *words, u32 *flags)
{
    if (m < 1 || k < 1 || m > 64 || k > 64) return -1;
    if (point >= 0 && (unit < 0 || unit >= k || !bc_point_exists(point, m))) return -2;
    const Plan pl(mi, m, mo, k);
    for (int o = 0; o < k; o++)
        if ((unsigned __int128)pl.q[o] * (u64)m >> 64) return -3;
    for (size_t i = 0; i < n; i++)
        for (int o = 0; o < k; o++)
            words[(size_t)o * n + i] = bc_checked_fast(m, [&](int j) { return in[(size_t)j * n + i]; }, [&](int j) { return pl.fast[(size_t)j * k + o]; }, pl.q[o],
                                                       res64(pl.q[o]), pl.q[o] * (u64)m, flags[(size_t)o * n + i], fault_at(point, unit, bit, o));
    return 0;
}

// k_bconv_fast
int emu_bc_fast_plain(const u64 *mi, int m, const u64 *mo, int k, const u64 *in, size_t n, u64 *words)
{
    if (m < 1 || k < 1 || m > 64 || k > 64) return -1;
    const Plan pl(mi, m, mo, k);
    for (size_t i = 0; i < n; i++)
        for (int o = 0; o < k; o++) {
            u64 total = 0;
            for (int j = 0; j < m; j++) total += mulmod_shoup(in[(size_t)j * n + i], pl.fast[(size_t)j * k + o].a, pl.fast[(size_t)j * k + o].b, pl.q[o]);
            words[(size_t)o * n + i] = total;
        }
    return 0;
}

} // extern "C"
