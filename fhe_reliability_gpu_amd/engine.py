"""Python host over the C ABI (``_lib``): device buffers, table sets and the
reference's Python-level operator names, so that code written against
``motivation/{ntt,baseConv,bsgs}.py``, ``rfhe_framewk/src/{ntt,negaclic_ntt,baseConv}.py``
and ``reliability_test/four_step_ntt_prot.py`` can switch to the GPU engine by
changing an import.  Every function here ends in HIP kernel launches; nothing is
computed on the CPU apart from packing/unpacking lists.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import check, lib, p64, u64, vp

_U64 = np.uint64

# seals of rows at rest (seal_check.hpp): the modulus of the two sums, and the flag bits of a verification
SEAL_P = (1 << 61) - 1
SEAL_SUM, SEAL_RANGE = 1, 2
# outcomes of a repair, per row (FHE_SEAL_* of fhe_mi355x.h): word 0 of a report record {outcome, index, word before, word after}
SEAL_CLEAN, SEAL_REPAIRED, SEAL_UNCORRECTABLE, SEAL_TRANSIENT, SEAL_SUSPECT = 0, 1, 2, 3, 4


def _arr(x) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(x, dtype=_U64))


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(p64)


class Engine:
    """One HIP device + stream (``phantom::util::cuda_stream_wrapper``, ntt_test.cu:40-41)."""

    def __init__(self, device: int = 0):
        h = vp()
        check(lib.fhe_ctx_create(device, C.byref(h)))
        self._h = h
        self.device = device
        s = vp()
        check(lib.fhe_ctx_stream(h, C.byref(s)))
        self.stream = s

    def set_option(self, name: str, value: int):
        """``ntt_mode`` (0 two launches / 1 fused), ``fused_dist``, ``fused_wgs`` -- tuning only."""
        check(lib.fhe_ctx_set_option(self._h, name.encode(), int(value)))

    def trace(self, enable: bool = True):
        """Start (and clear) / stop the operation trace (profile_framewk trace-line format)."""
        check(lib.fhe_ctx_trace(self._h, 1 if enable else 0))

    def trace_text(self) -> str:
        n = C.c_size_t()
        check(lib.fhe_ctx_trace_read(self._h, None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value + 1)
        check(lib.fhe_ctx_trace_read(self._h, buf, n.value + 1, None))
        return buf.value.decode("utf-8")

    def inject_fault_tensor_sealed(self, operand: int, row: int = 0, coeff: int = 0, bit: int = 0):
        """One-shot test hook of ``KeySwitch.tensor_sealed`` / ``hmult_sealed_fused``: flip ``bit`` of word ``coeff`` of row ``row``
        of operand 0..3 (a0, a1, b0, b1) in the register as the next such call loads it, before the window, the digest and the
        product read it; memory stays clean.  A negative ``operand`` disarms."""
        check(lib.fhe_ctx_inject_fault_tensor_sealed(self._h, operand, row, coeff, bit))

    def inject_fault_keyswitch_sealed(self, key_row: int, coeff: int = 0, bit: int = 0):
        """One-shot test hook of ``KeySwitch.apply_sealed`` / ``rotate_sealed_fused`` / ``hmult_sealed_fused_key``: flip ``bit`` of
        word ``coeff`` of key row ``key_row = (d * 2 + h) * M + j`` in the register as the next such call's inner product loads it,
        before the window, the digest and the product read it; memory stays clean.  A negative ``key_row`` disarms."""
        check(lib.fhe_ctx_inject_fault_keyswitch_sealed(self._h, key_row, coeff, bit))

    def inject_fault_galois_sealed(self, rot: int, point: int, row: int = 0, coeff: int = 0, bit: int = 0):
        """One-shot test hook of ``automorphism_sealed`` (``rot`` = 0) / ``KeySwitch.rotate_hoisted_sealed`` (c0 in rotation ``rot``):
        at destination word ``coeff`` of row ``row``, point 0 flips ``bit`` of the gathered word in the register, before both digests
        and the store; point 1 flips ``bit`` (< log N) of its source index, before the load.  Memory stays clean.  A negative
        ``point`` disarms."""
        check(lib.fhe_ctx_inject_fault_galois_sealed(self._h, rot, point, row, coeff, bit))

    def inject_fault_ntt_sealed(self, row: int, coeff: int = 0, bit: int = 0):
        """One-shot test hook of ``NttTables.intt_sealed`` / ``ntt_sealed`` / ``intt_sealed_out`` / ``KeySwitch.apply_sealed_in`` /
        ``rotate_sealed_in``: flip ``bit`` of
        word ``coeff`` of row ``row`` of the sealed transform's input (a row of the source, of ``c``, of sigma(c1)) in the
        register as the next such call's first launch loads it, before the window, the digest and the conversion read it; memory
        stays clean.  A negative ``row`` disarms."""
        check(lib.fhe_ctx_inject_fault_ntt_sealed(self._h, row, coeff, bit))

    def inject_fault_polymul_sealed(self, operand: int, row: int = 0, coeff: int = 0, bit: int = 0):
        """One-shot test hook of ``Abft.polymul_sealed``: flip ``bit`` of word ``coeff`` of row ``row`` of factor ``operand`` (0 = a,
        1 = b) in the register as the next such call's loading launch takes it, before the window, the digest and the conversion
        read it; memory stays clean.  A negative ``operand`` disarms.  ``Abft.polymul_checked`` does not take it."""
        check(lib.fhe_ctx_inject_fault_polymul_sealed(self._h, operand, row, coeff, bit))

    def inject_fault_subscale_sealed(self, point: int, row: int = 0, coeff: int = 0, bit: int = 0):
        """One-shot test hook of ``KeySwitch.rescale_sealed`` / ``hmult_sealed_out`` / ``rotate_sealed_out``: point 0 flips ``bit`` of
        word ``coeff`` of input row ``row = part * L + l`` (l < L - 1; ``rescale_sealed`` only) in the register as the sealed tail
        loads it, before the window, the digest and the arithmetic read it; point 1 flips ``bit`` of word ``coeff`` of output row
        ``row = part * limbs + l`` in the register after its digest and before its store.  A negative ``point`` disarms."""
        check(lib.fhe_ctx_inject_fault_subscale_sealed(self._h, point, row, coeff, bit))

    def check(self):
        """Synchronise and raise if a fused-NTT launch reported a timed-out wait."""
        check(lib.fhe_ctx_check(self._h))

    def close(self):
        if getattr(self, "_h", None):
            lib.fhe_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- memory ------------------------------------------------------------
    def alloc(self, n_words: int) -> "DeviceArray":
        return DeviceArray(self, n_words)

    def upload(self, host) -> "DeviceArray":
        a = _arr(host)
        d = DeviceArray(self, a.size)
        d.shape = a.shape
        check(lib.fhe_h2d(self._h, d.ptr, a.ctypes.data, a.nbytes, None))
        self.sync()  # the NumPy temporary must outlive the async copy
        return d

    def sync(self, stream=None):
        check(lib.fhe_sync(self._h, stream))

    # -- tables ------------------------------------------------------------
    def tables(self, log_n: int, moduli: Sequence[int]) -> "NttTables":
        return NttTables(self, log_n, moduli)

    def tables_from_roots(self, log_n: int, moduli: Sequence[int], root_powers, force_path: int = -1) -> "NttTables":
        return NttTables(self, log_n, moduli, root_powers=root_powers, force_path=force_path)


class DeviceArray:
    """uint64 words in HBM, owned through fhe_alloc/fhe_free (make_cuda_auto_ptr, ntt_test.cu:88)."""

    def __init__(self, eng: Engine, n_words: int):
        self.eng = eng
        self.size = int(n_words)
        self.shape = (self.size,)
        p = vp()
        check(lib.fhe_alloc(eng._h, self.size * 8, C.byref(p)))
        self.ptr = p

    def download(self) -> np.ndarray:
        out = np.empty(self.size, dtype=_U64)
        check(lib.fhe_d2h(self.eng._h, out.ctypes.data, self.ptr, out.nbytes, None))
        self.eng.sync()
        return out.reshape(self.shape)

    def copy_from(self, other: "DeviceArray"):
        check(lib.fhe_d2d(self.eng._h, self.ptr, other.ptr, min(self.size, other.size) * 8, None))

    def free(self):
        if self.ptr:
            lib.fhe_free(self.eng._h, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            if self.eng._h:
                self.free()
        except Exception:
            pass


def _flag_buffer(eng: Engine, n: int) -> DeviceArray:
    """``n`` uint32 flag words (packed in a u64 buffer) holding a pattern no check leaves behind: the checked calls clear or
    write every word themselves."""
    return eng.upload(np.full((n + 1) // 2, 0xA5A5A5A5A5A5A5A5, dtype=_U64))


def _read_flags(flags: DeviceArray, n: int, stream=None) -> np.ndarray:
    """The ``n`` flag words once the call's stream (when one was given) has finished: a view into the download, to be copied."""
    if stream is not None:
        flags.eng.sync(stream)
    return flags.download().view(np.uint32)[:n]


def _checked_flags(eng: Engine, n: int, call, stream=None) -> np.ndarray:
    """The ``n`` flag words (uint32, an array of its own) of the checked call ``call(flags)``, which returns the C status."""
    flags = _flag_buffer(eng, n)
    check(call(flags))
    return _read_flags(flags, n, stream).copy()


def create_moduli(N: int, bits: Sequence[int]) -> List[int]:
    """``CoeffModulus::Create(N, {bits...})`` (reliability_test/ntt_test.cu:44)."""
    b = (C.c_int * len(bits))(*bits)
    out = (u64 * len(bits))()
    check(lib.fhe_moduli_create(N, b, len(bits), out))
    return [int(x) for x in out]


def min_primitive_root(q: int, order: int) -> int:
    r = u64()
    check(lib.fhe_min_primitive_root(q, order, C.byref(r)))
    return int(r.value)


def root_powers(q: int, log_n: int, shoup: bool = False):
    """``NTT::get_from_root_powers[_shoup]`` (ntt_test.cu:60-64)."""
    rp = np.zeros(1 << log_n, dtype=_U64)
    sh = np.zeros(1 << log_n, dtype=_U64)
    check(lib.fhe_root_powers(q, log_n, _ptr(rp), _ptr(sh)))
    return (rp, sh) if shoup else rp


class NttTables:
    """``DModulus[]`` + ``DNTTTable`` of a limb set (ntt_test.cu:47-69)."""

    def __init__(self, eng: Engine, log_n: int, moduli: Sequence[int], root_powers=None, force_path: int = -1):
        self.eng = eng
        self.log_n = log_n
        self.N = 1 << log_n
        self.moduli = [int(q) for q in moduli]
        q = _arr(self.moduli)
        h = vp()
        if root_powers is None:
            check(lib.fhe_ntt_tables_create(eng._h, log_n, _ptr(q), q.size, C.byref(h)))
        else:
            rp = _arr(root_powers).reshape(q.size, self.N)
            check(lib.fhe_ntt_tables_create_from_roots(eng._h, log_n, _ptr(q), q.size, _ptr(rp), force_path, C.byref(h)))
        self._h = h
        paths = (C.c_int * q.size)()
        psi = (u64 * q.size)()
        check(lib.fhe_ntt_tables_info(h, None, None, paths, psi))
        self.paths = list(paths)
        self.psi = [int(x) for x in psi]

    def __len__(self):
        return len(self.moduli)

    # nwt_2d_radix8_forward_inplace (ntt_test.cu:95): d is [n_poly][limbs][N]
    def forward(self, d: DeviceArray, limbs: Optional[int] = None, start: int = 0, n_poly: int = 1, stream=None):
        limbs = len(self) - start if limbs is None else limbs
        check(lib.fhe_ntt_forward_batch(self.eng._h, d.ptr, self._h, n_poly, limbs, start, stream))

    def inverse(self, d: DeviceArray, limbs: Optional[int] = None, start: int = 0, n_poly: int = 1, stream=None):
        limbs = len(self) - start if limbs is None else limbs
        check(lib.fhe_ntt_inverse_batch(self.eng._h, d.ptr, self._h, n_poly, limbs, start, stream))

    def modmul(self, c: DeviceArray, a: DeviceArray, b: DeviceArray, limbs=None, start=0, n_poly=1, acc=False, stream=None):
        limbs = len(self) - start if limbs is None else limbs
        f = lib.fhe_modmul_acc if acc else lib.fhe_modmul
        check(f(self.eng._h, c.ptr, a.ptr, b.ptr, self._h, n_poly, limbs, start, stream))

    def modmul_checked(self, c: DeviceArray, a: DeviceArray, b: DeviceArray, limbs=None, start=0, n_poly=1, acc=False,
                       stream=None) -> np.ndarray:
        """``modmul`` with every word checked; the words are ``modmul``'s, bit for bit.  Returns flags[poly * limbs + l] (uint32):
        1 = residue identity a b (+ o) = k q + c failed modulo 2^32 - 1, 2 = a result or a reduction intermediate out of its
        window, 4 = an operand (or, with ``acc``, the old word) not canonical, which the check cannot cover.

        The per-element protections of rfhe_framewk/src/barrett_final.py (Intra, Range, Sum) in one identity, with a 32-bit
        fold instead of the reference's 4-10-bit ones; the fold checksum that four_step_ntt_protected.py:102-120 puts on the
        element-wise stage of its pipeline, here per word (residue_check.hpp)."""
        limbs = len(self) - start if limbs is None else limbs
        n = n_poly * limbs
        f = lib.fhe_modmul_acc_checked if acc else lib.fhe_modmul_checked
        return _checked_flags(self.eng, n, lambda fl: f(self.eng._h, c.ptr, a.ptr, b.ptr, self._h, n_poly, limbs, start, fl.ptr, stream), stream)

    def modadd_checked(self, c: DeviceArray, a: DeviceArray, b: DeviceArray, limbs=None, start=0, n_poly=1, stream=None) -> np.ndarray:
        """c = (a + b) mod q per limb with every word checked; the words are ``fhe_modadd``'s, bit for bit.  Returns
        flags[poly * limbs + l] (uint32): 1 = r(c) + e r(q) == r(a) + r(b) failed modulo 2^32 - 1 (e = the conditional subtraction),
        2 = the word out of its window, 4 = an operand not canonical, which the check cannot cover (bsgs_check.hpp)."""
        limbs = len(self) - start if limbs is None else limbs
        n = n_poly * limbs
        return _checked_flags(self.eng, n, lambda fl: lib.fhe_modadd_checked(self.eng._h, c.ptr, a.ptr, b.ptr, self._h, n_poly, limbs, start, fl.ptr, stream),
                              stream)

    def scalar_affine_checked(self, c: DeviceArray, a: DeviceArray, mul=None, add=None, limbs=None, start=0, n_poly=1, stream=None) -> np.ndarray:
        """c = a * mul[l] + add[l] mod q_l per limb (``mul`` None: 1, ``add`` None: 0; c may be a) with every word checked; the words
        are ``fhe_scalar_affine``'s, bit for bit.  Returns flags[poly * limbs + l] (uint32): 1 = a s (+ o) = k q + c failed modulo
        2^32 - 1, 2 = the word or the quotient out of its window, 4 = a word of ``a`` not canonical, which the check cannot cover
        (scalar_check.hpp)."""
        limbs = len(self) - start if limbs is None else limbs
        n = n_poly * limbs
        m = _arr(mul) if mul is not None else None
        o = _arr(add) if add is not None else None
        return _checked_flags(self.eng, n, lambda fl: lib.fhe_scalar_affine_checked(
            self.eng._h, c.ptr, a.ptr, _ptr(m) if m is not None else None, _ptr(o) if o is not None else None, self._h, n_poly, limbs, start, fl.ptr,
            stream), stream)

    def seal(self, d: DeviceArray, limbs=None, start=0, n_poly=1, stream=None) -> DeviceArray:
        """The seals of the rows of ``d`` = [n_poly][limbs][N]: a device array ``[n_poly * limbs][2]`` of (S0, S1) with
        S0 = sum x_j, S1 = sum (j + 1) x_j modulo 2^61 - 1, canonical.  An integrity record that travels with a ciphertext or key
        between calls (``seal_verify``, ``KeySwitch.hmult_sealed`` / ``rotate_sealed``): the checked calls do not cover faults
        already in their inputs -- the flips of reliability_test/dotprod_test.cu:31-61."""
        limbs = len(self) - start if limbs is None else limbs
        out = self.eng.alloc(n_poly * limbs * 2)
        out.shape = (n_poly * limbs, 2)
        check(lib.fhe_seal(self.eng._h, out.ptr, d.ptr, self._h, n_poly, limbs, start, stream))
        return out

    def seal_verify(self, d: DeviceArray, seal: DeviceArray, limbs=None, start=0, n_poly=1, stream=None) -> np.ndarray:
        """Sweep the rows of ``d`` against ``seal``: flags[poly * limbs + l] (uint32), ``SEAL_SUM`` (1) = a sum differs,
        ``SEAL_RANGE`` (2) = some word >= q_l.  A change confined to one or two words of a row is caught with certainty
        (seal_check.hpp)."""
        limbs = len(self) - start if limbs is None else limbs
        return _checked_flags(self.eng, n_poly * limbs, lambda fl: lib.fhe_seal_verify(self.eng._h, d.ptr, seal.ptr, self._h, n_poly, limbs, start, fl.ptr,
                                                                                       stream), stream)

    def intt_sealed(self, src: DeviceArray, seal: Optional[DeviceArray], abft: "Abft", dst: Optional[DeviceArray] = None, limbs=None, start=0, n_poly=1,
                    stream=None):
        """The inverse NTT of the rows of ``src`` with their seal verified on the transform's own load: ``(dst, flags)``,
        ``flags`` uint32 ``[2][rows]`` -- block 0 the seal verdict per row with ``seal_verify``'s bits (``SEAL_SUM`` the row as the
        transform loaded it is not the row that was sealed, ``SEAL_RANGE`` a word >= q_l), block 1 ``Abft.inverse_checked``'s flag.
        ``dst`` None: a new array (out of place, no copy; ``src`` is only read); ``dst`` may be ``src`` (in place).  ``seal`` from
        ``seal`` (None: not compared, the window still is).  The words are ``intt``'s, bit for bit; a raised seal flag does not stop
        the call.  Whole-batch launches only: never cut into sub-batches."""
        call = lambda h, d, s, t, a, n_poly, limbs, start, seal_src, seal_dst, fl, st: lib.fhe_ntt_inverse_sealed(h, d, s, t, a, n_poly, limbs, start, seal_src, fl, st)
        dst, _, f = self._sealed_io(call, src, seal, abft, dst, False, limbs, start, n_poly, stream)
        return dst, f

    def _sealed_io(self, call, src, seal, abft, dst, seal_out, limbs, start, n_poly, stream):
        limbs = len(self) - start if limbs is None else limbs
        rows = n_poly * limbs
        if dst is None:
            dst = self.eng.alloc(src.size)
            dst.shape = src.shape
        seal_dst = None
        if seal_out:
            seal_dst = self.eng.alloc(rows * 2)
            seal_dst.shape = (rows, 2)
        f = _checked_flags(self.eng, 2 * rows, lambda fl: call(
            self.eng._h, dst.ptr, src.ptr, self._h, abft._h, n_poly, limbs, start, seal.ptr if seal is not None else None,
            seal_dst.ptr if seal_dst is not None else None, fl.ptr, stream), stream)
        return dst, seal_dst, f.reshape(2, rows)

    def ntt_sealed(self, src: DeviceArray, seal: Optional[DeviceArray], abft: "Abft", dst: Optional[DeviceArray] = None, seal_out: bool = True, limbs=None,
                   start=0, n_poly=1, stream=None):
        """The forward NTT of the rows of ``src`` with their seal verified on the transform's own load and the seal of the result
        written from the words the transform stores: ``(dst, seal_dst, flags)``.  ``flags`` uint32 ``[2][rows]`` -- block 0 the input
        seal verdict per row with ``seal_verify``'s bits, block 1 ``Abft.forward_checked``'s flag.  ``seal_dst`` is ``[rows][2]``,
        ``seal``'s of ``dst`` word for word on a row with no raised flag and ``{~0, ~0}`` otherwise: a raised row leaves the call with
        a seal that can never verify.  ``seal_out`` False: no output digest, ``seal_dst`` is None.  ``dst`` None: a new array (out
        of place, no copy; ``src`` is only read); ``dst`` may be ``src`` (in place).  ``seal`` None: not compared, the window still
        is.  The words are ``forward``'s, bit for bit; a raised flag does not stop the call.  Whole-batch launches only."""
        return self._sealed_io(lib.fhe_ntt_forward_sealed, src, seal, abft, dst, seal_out, limbs, start, n_poly, stream)

    def intt_sealed_out(self, src: DeviceArray, seal: Optional[DeviceArray], abft: "Abft", dst: Optional[DeviceArray] = None, seal_out: bool = True, limbs=None,
                        start=0, n_poly=1, stream=None):
        """``intt_sealed`` that also writes the seal of its result from the words it stores: ``(dst, seal_dst, flags)`` as
        ``ntt_sealed``, over ``inverse``'s words and ``Abft.inverse_checked``'s flag."""
        return self._sealed_io(lib.fhe_ntt_inverse_sealed_out, src, seal, abft, dst, seal_out, limbs, start, n_poly, stream)

    def seal_locator(self, d: DeviceArray, limbs=None, start=0, n_poly=1, stream=None) -> DeviceArray:
        """The locator sums of the rows of ``d``: a device array ``[n_poly * limbs]`` of S2 = sum (j + 1)^2 x_j modulo 2^61 - 1,
        canonical.  Kept beside the seal, it makes a row's three sums a single-error-correcting code (``seal_repair``)."""
        limbs = len(self) - start if limbs is None else limbs
        out = self.eng.alloc(n_poly * limbs)
        check(lib.fhe_seal_locator(self.eng._h, out.ptr, d.ptr, self._h, n_poly, limbs, start, stream))
        return out

    def seal_repair(self, d: DeviceArray, seal: DeviceArray, locator: DeviceArray, limbs=None, start=0, n_poly=1, stream=None):
        """``seal_verify`` followed by the repair of every flagged row, in place, on the device: ``(flags, report)``.  ``report`` is
        uint64 ``[rows][4]`` = {outcome, index, word before, word after} with the outcomes ``SEAL_CLEAN`` / ``SEAL_REPAIRED`` /
        ``SEAL_UNCORRECTABLE`` / ``SEAL_TRANSIENT`` / ``SEAL_SUSPECT``; ``flags`` are ``seal_verify``'s, cleared again for repaired
        and transient rows.  One corrupted word per row, any 64-bit pattern, is restored exactly; two corrupted words in a row are
        never written to; a corrupted seal or locator word never causes a write (seal_check.hpp)."""
        limbs = len(self) - start if limbs is None else limbs
        rows = n_poly * limbs
        report = self.eng.upload(np.full(max(rows, 1) * 4, 0xA5A5A5A5A5A5A5A5, dtype=_U64))
        flags = _checked_flags(self.eng, rows, lambda fl: lib.fhe_seal_repair(self.eng._h, d.ptr, seal.ptr, locator.ptr, self._h, n_poly, limbs, start,
                                                                              fl.ptr, report.ptr, stream), stream)
        return flags, report.download()[:rows * 4].reshape(rows, 4)

    def _carried(self, f, c, a, b, seal_a, seal_b, seal_c, locators, limbs, start, n_poly, stream):
        limbs = len(self) - start if limbs is None else limbs
        rows = n_poly * limbs
        if seal_c is None:
            seal_c = self.eng.alloc(rows * 2)
            seal_c.shape = (rows, 2)
        loc = list(locators) if locators is not None else [None] * 3
        if locators is not None and len(loc) == 2:
            loc.append(self.eng.alloc(rows))
        lp = [x.ptr if x is not None else None for x in loc]
        flags = _checked_flags(self.eng, rows, lambda fl: f(self.eng._h, c.ptr, a.ptr, b.ptr, seal_c.ptr, seal_a.ptr, seal_b.ptr, lp[2], lp[0], lp[1], self._h,
                                                            n_poly, limbs, start, fl.ptr, stream), stream)
        return (seal_c, flags) if locators is None else (seal_c, loc[2], flags)

    def modadd_sealed(self, c: DeviceArray, a: DeviceArray, b: DeviceArray, seal_a: DeviceArray, seal_b: DeviceArray, seal_c: Optional[DeviceArray] = None,
                      locators=None, limbs=None, start=0, n_poly=1, stream=None):
        """c = (a + b) mod q per limb with the operands' seals carried to the result in the same sweep: ``(seal_c, flags)``, or
        ``(seal_c, locator_c, flags)`` with ``locators = (locator_a, locator_b[, locator_c])``.  The words are ``fhe_modadd``'s, bit
        for bit.  The seal is linear: S_i(c) = S_i(a) + S_i(b) - q E_i with E_i the weighted count of the wraps, so the digest of
        the words about to be stored is held against the sums predicted from ``seal_a`` and ``seal_b``; flags[poly * limbs + l]
        (uint32): ``SEAL_SUM`` (1) = they differ -- an operand word that is not the sealed one, a fault in the adder or in the wrap
        count -- ``SEAL_RANGE`` (2) = an operand word >= q_l.  ``seal_c`` always receives the predicted sums, so a raised row stays
        raised through later carried adds and a fault after the digest is caught by the next verification.  ``c`` may be ``a`` or
        ``b`` and ``seal_c`` may be ``seal_a`` or ``seal_b`` (seal_carry.hpp)."""
        return self._carried(lib.fhe_modadd_sealed, c, a, b, seal_a, seal_b, seal_c, locators, limbs, start, n_poly, stream)

    def modsub_sealed(self, c: DeviceArray, a: DeviceArray, b: DeviceArray, seal_a: DeviceArray, seal_b: DeviceArray, seal_c: Optional[DeviceArray] = None,
                      locators=None, limbs=None, start=0, n_poly=1, stream=None):
        """c = (a - b) mod q per limb, otherwise ``modadd_sealed``: S_i(c) = S_i(a) - S_i(b) + q E_i; the words are ``fhe_modsub``'s."""
        return self._carried(lib.fhe_modsub_sealed, c, a, b, seal_a, seal_b, seal_c, locators, limbs, start, n_poly, stream)

    def polymul(self, c: DeviceArray, a: DeviceArray, b: DeviceArray, limbs=None, start=0, n_poly=1, stream=None):
        limbs = len(self) - start if limbs is None else limbs
        check(lib.fhe_polymul(self.eng._h, c.ptr, a.ptr, b.ptr, self._h, n_poly, limbs, start, stream))

    def close(self):
        if getattr(self, "_h", None) and self.eng._h:
            lib.fhe_ntt_tables_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------
# Reference-named operators (lists in, lists out)
# ---------------------------------------------------------------------------
_default_engine: Optional[Engine] = None


def default_engine() -> Engine:
    global _default_engine
    if _default_engine is None:
        _default_engine = Engine(0)
    return _default_engine


def _log2(n: int) -> int:
    if n < 2 or n & (n - 1):
        raise ValueError("length must be a power of two >= 2")
    return n.bit_length() - 1


def _cyclic(a, mod, root, convention, inverse, eng):
    eng = eng or default_engine()
    h = _arr(a)
    vecs = h.reshape(-1, h.shape[-1])
    d = eng.upload(vecs)
    s = eng.alloc(vecs.size)
    check(lib.fhe_ntt_cyclic(eng._h, d.ptr, s.ptr, _log2(vecs.shape[1]), vecs.shape[0], mod, root, convention, inverse, None))
    out = d.download().reshape(h.shape)
    return out


def ntt(a, mod: int, root: int, eng: Optional[Engine] = None) -> List[int]:
    """``ntt(a, mod, root)`` of motivation/ntt.py:8-32 (``root`` generates Z_mod*)."""
    return [int(x) for x in _cyclic(a, mod, root, 0, 0, eng)]


def intt(a, mod: int, root: int, eng: Optional[Engine] = None) -> List[int]:
    """``intt(a, mod, root)`` of motivation/bsgs.py:31-36."""
    return [int(x) for x in _cyclic(a, mod, root, 0, 1, eng)]


def ntt_nthroot(a, root: int, mod: int, eng: Optional[Engine] = None) -> List[int]:
    """``ntt(a, root, mod)`` of rfhe_framewk/src/negaclic_ntt.py:38-57 (``root`` is an n-th root)."""
    return [int(x) for x in _cyclic(a, mod, root, 1, 0, eng)]


def intt_nthroot(a, root: int, mod: int, eng: Optional[Engine] = None) -> List[int]:
    """``intt(a, root, mod)`` of rfhe_framewk/src/negaclic_ntt.py:77-83."""
    return [int(x) for x in _cyclic(a, mod, root, 1, 1, eng)]


def _psi_tables(eng: Engine, n: int, psi: int, mod: int) -> NttTables:
    log_n = _log2(n)
    rp = np.zeros(n, dtype=_U64)
    p = 1
    for i in range(n):
        rp[int(f"{i:0{log_n}b}"[::-1], 2)] = p
        p = p * psi % mod
    return eng.tables_from_roots(log_n, [mod], rp)


def negacyclic_ntt(a, psi: int, mod: int, eng: Optional[Engine] = None) -> List[int]:
    """``negacyclic_ntt(a, psi, mod)`` of rfhe_framewk/src/negaclic_ntt.py:86-92 (natural-order output)."""
    eng = eng or default_engine()
    n = len(a)
    t = _psi_tables(eng, n, psi, mod)
    d = eng.upload(a)
    t.forward(d)
    out = eng.alloc(n)
    check(lib.fhe_bitrev_permute(eng._h, out.ptr, d.ptr, t.log_n, 1, None))
    return [int(x) for x in out.download()]


def negacyclic_intt(A, psi: int, mod: int, eng: Optional[Engine] = None) -> List[int]:
    """``negacyclic_intt(A, psi, mod)`` of rfhe_framewk/src/negaclic_ntt.py:102-109."""
    eng = eng or default_engine()
    n = len(A)
    t = _psi_tables(eng, n, psi, mod)
    src = eng.upload(A)
    d = eng.alloc(n)
    check(lib.fhe_bitrev_permute(eng._h, d.ptr, src.ptr, t.log_n, 1, None))
    t.inverse(d)
    return [int(x) for x in d.download()]


def poly_mul_negacyclic_ntt(a, b, psi: int, mod: int, eng: Optional[Engine] = None) -> List[int]:
    """``poly_mul_negacyclic_ntt`` of rfhe_framewk/src/negaclic_ntt.py:123-127."""
    eng = eng or default_engine()
    t = _psi_tables(eng, len(a), psi, mod)
    da, db = eng.upload(a), eng.upload(b)
    t.polymul(da, da, db)
    return [int(x) for x in da.download()]


def four_step_ntt(a, N: int, mod: int = 998244353, g: int = 3, n1: Optional[int] = None, eng: Optional[Engine] = None):
    """``four_step_ntt(a, N, mod, g)`` of reliability_test/four_step_ntt_prot.py:71-109.
    ``n1`` defaults to sqrt(N) as in the reference (:73-75); any power-of-two split is accepted.  ``a`` may be a batch
    ([n_vec][N]): one call transforms all vectors (two launches in total) and a list of lists comes back."""
    eng = eng or default_engine()
    log_n = _log2(N)
    arr = _arr(a)
    if arr.ndim == 2:
        if n1 is None:
            n1 = 1 << (log_n // 2)
        h = vp()
        check(lib.fhe_fourstep_create(eng._h, n1, N // n1, mod, g, C.byref(h)))
        try:
            src = eng.upload(arr)
            dst = eng.alloc(arr.size)
            check(lib.fhe_fourstep_ntt_batch(eng._h, dst.ptr, src.ptr, h, arr.shape[0], None))
            return dst.download().reshape(arr.shape).tolist()
        finally:
            lib.fhe_fourstep_destroy(h)
    if n1 is None:
        n1 = 1 << (log_n // 2)
        if n1 * n1 != N:
            raise AssertionError("N must be a perfect square unless n1 is given")  # four_step_ntt_prot.py:74
    n2 = N // n1
    h = vp()
    check(lib.fhe_fourstep_create(eng._h, n1, n2, mod, g, C.byref(h)))
    try:
        src = eng.upload(a)
        dst = eng.alloc(N)
        check(lib.fhe_fourstep_ntt(eng._h, dst.ptr, src.ptr, h, None))
        return [int(x) for x in dst.download()]
    finally:
        lib.fhe_fourstep_destroy(h)


class FourStep:
    """Four-step plan of N = n1 * n2 points (reliability_test/four_step_ntt_prot.py:71-79) with the unchecked and the
    ABFT-checked natural-order transform of batches ``[n_vec][N]``.  One plan, one stream at a time."""

    def __init__(self, eng: Engine, n1: int, n2: int, mod: int = 998244353, g: int = 3):
        self.eng, self.n1, self.n2, self.N, self.mod, self.g = eng, n1, n2, n1 * n2, mod, g
        h = vp()
        check(lib.fhe_fourstep_create(eng._h, n1, n2, mod, g, C.byref(h)))
        self._h = h

    def prepare_checked(self, stream=None):
        """Build the weight tables of the checked calls now (they do it on first use otherwise)."""
        check(lib.fhe_fourstep_prepare_checked(self.eng._h, self._h, stream))

    def ntt(self, src: DeviceArray, dst: DeviceArray, n_vec: int = 1, stream=None):
        """``four_step_ntt`` of every vector (four_step_ntt_prot.py:71-109); ``dst`` may be ``src``."""
        check(lib.fhe_fourstep_ntt_batch(self.eng._h, dst.ptr, src.ptr, self._h, n_vec, stream))

    def checksum(self, d: DeviceArray, side: int, n_vec: int = 1, stream=None) -> np.ndarray:
        """Per vector: sum u x over input vectors (side 0) or sum v y over output vectors (side 1) modulo ``mod``, the two sides
        of the whole-transform check (``fhe_fourstep_checksum``)."""
        out = self.eng.alloc(n_vec)
        check(lib.fhe_fourstep_checksum(self.eng._h, self._h, side, d.ptr, out.ptr, n_vec, stream))
        if stream is not None:
            self.eng.sync(stream)
        return out.download()

    def ntt_checked(self, src: DeviceArray, dst: DeviceArray, n_vec: int = 1, stream=None) -> np.ndarray:
        """``ntt`` with the whole-transform check sum u x == sum v y riding on the launches; the words are ``ntt``'s, bit for
        bit.  Returns flags[n_vec] (uint32, 0 / 1)."""
        return _checked_flags(self.eng, n_vec, lambda fl: lib.fhe_fourstep_ntt_checked(self.eng._h, dst.ptr, src.ptr, self._h, n_vec, fl.ptr, stream), stream)

    def ntt_checked_phases(self, src: DeviceArray, dst: DeviceArray, n_vec: int = 1, stream=None) -> np.ndarray:
        """``ntt`` with one check per phase (N >= 2^13): flags[n_vec, 3] = launch 1 (the reference's stage 1), the hand-off
        between the launches, launch 2 (stage 2)."""
        return _checked_flags(self.eng, 3 * n_vec, lambda fl: lib.fhe_fourstep_ntt_checked_phases(self.eng._h, dst.ptr, src.ptr, self._h, n_vec, fl.ptr, stream),
                              stream).reshape(n_vec, 3)

    def close(self):
        if getattr(self, "_h", None) and self.eng._h:
            lib.fhe_fourstep_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def four_step_with_protection_vector(a, N: int, mod: int = 998244353, g: int = 3, n1: Optional[int] = None, eng: Optional[Engine] = None):
    """``four_step_with_protection_vector(a, N, mod, g)`` of reliability_test/four_step_ntt_prot.py:196-252: the four-step
    transform of ``a`` with its stages checked.  Returns ``(y, checks)``; for N >= 2^13
    ``checks = {"stage1": {"ok": bool}, "handoff": {"ok": bool}, "stage2": {"ok": bool}}`` (the engine's two launches are the
    reference's two stages, and the buffer between them is checked as well), below that ``{"transform": {"ok": bool}}``.

    Differences from the reference: the checksums are weighted sums with the weights of ``generate_weights``
    (rfhe_framewk/src/negaclic_ntt.py:7-13) on the output, their transposed images on the hand-off and on the input, instead
    of the reference's all-ones vectors, under which only x_0 would be weighed (W 1 = N delta_0; the reference calls its own
    check weak); and the ``lhs`` / ``rhs`` values of the reference's dictionaries are not returned, the comparison happens on
    the device."""
    eng = eng or default_engine()
    log_n = _log2(N)
    if n1 is None:
        n1 = 1 << (log_n // 2)
    fs = FourStep(eng, n1, N // n1, mod, g)
    try:
        src = eng.upload(_arr(a).reshape(N))
        dst = eng.alloc(N)
        if log_n >= 13:
            f = fs.ntt_checked_phases(src, dst)[0]
            checks = {"stage1": {"ok": not f[0]}, "handoff": {"ok": not f[1]}, "stage2": {"ok": not f[2]}}
        else:
            checks = {"transform": {"ok": not fs.ntt_checked(src, dst)[0]}}
        return [int(x) for x in dst.download()], checks
    finally:
        fs.close()


class BaseConv:
    """Base-conversion plan for (moduli_in -> moduli_out)."""

    def __init__(self, eng: Engine, moduli_in: Sequence[int], moduli_out: Sequence[int]):
        self.eng, self.m, self.k = eng, len(moduli_in), len(moduli_out)
        mi, mo = _arr(moduli_in), _arr(moduli_out)
        h = vp()
        check(lib.fhe_baseconv_create(eng._h, _ptr(mi), self.m, _ptr(mo), self.k, C.byref(h)))
        self._h = h

    def exact(self, out: DeviceArray, inp: DeviceArray, N: int, stream=None):
        check(lib.fhe_baseconv_exact(self.eng._h, out.ptr, inp.ptr, self._h, N, stream))

    def fast(self, out: DeviceArray, inp: DeviceArray, N: int, stream=None):
        check(lib.fhe_baseconv_fast(self.eng._h, out.ptr, inp.ptr, self._h, N, stream))

    def _checked(self, f, units, out, inp, N, stream):
        return _checked_flags(self.eng, units, lambda fl: f(self.eng._h, out.ptr, inp.ptr, self._h, N, fl.ptr, stream), stream)

    def exact_checked(self, out: DeviceArray, inp: DeviceArray, N: int, stream=None) -> np.ndarray:
        """``exact`` with every mixed-radix digit and every output word checked; the words are ``exact``'s, bit for bit.
        Returns flags (uint32) of shape ``(m + k,)``: ``flags[j]`` the digit recurrence of input limb j, ``flags[m + o]`` output
        limb o.  1 = residue identity (r_j A_j - sum c_l D_lj = K p_j + c_j, sum c_l E_lo = K q_o + out_o) failed modulo
        2^32 - 1, 2 = a digit or word out of its window, 4 = an input word >= p_j, which is folded but not checked.

        The stage motivation/baseConv.py perturbs, with the fold-residue and range detectors of
        rfhe_framewk/src/barrett_final.py carried through the sums (baseconv_check.hpp)."""
        return self._checked(lib.fhe_baseconv_exact_checked, self.m + self.k, out, inp, N, stream)

    def fast_checked(self, out: DeviceArray, inp: DeviceArray, N: int, stream=None) -> np.ndarray:
        """``fast`` with every output word checked (sum_j in_j C_jo = K q_o + out_o modulo 2^32 - 1, every reduced term below
        q_o, the word below m q_o); flags of shape ``(k,)``, bits as ``exact_checked`` (4 is never raised)."""
        return self._checked(lib.fhe_baseconv_fast_checked, self.k, out, inp, N, stream)

    def __del__(self):
        try:
            if self._h and self.eng._h:
                lib.fhe_baseconv_destroy(self._h)
        except Exception:
            pass


def base_conv_fixed(residue_arrays, moduli_in, moduli_out, eng: Optional[Engine] = None) -> List[List[int]]:
    """``base_conv_fixed`` of motivation/baseConv.py:67-83; returns ``[k][i]``."""
    eng = eng or default_engine()
    r = _arr(residue_arrays)
    N = r.shape[1]
    bc = BaseConv(eng, moduli_in, moduli_out)
    d = eng.upload(r)
    o = eng.alloc(len(moduli_out) * N)
    bc.exact(o, d, N)
    return o.download().reshape(len(moduli_out), N).tolist()


def bConv(residue_arrays, moduli, moduli_out, eng: Optional[Engine] = None) -> List[List[int]]:
    """``bConv`` of rfhe_framewk/src/baseConv.py:10-40; returns ``[i][k]`` like the reference."""
    eng = eng or default_engine()
    r = _arr(residue_arrays)
    N = r.shape[1]
    bc = BaseConv(eng, moduli, moduli_out)
    d = eng.upload(r)
    o = eng.alloc(len(moduli_out) * N)
    bc.fast(o, d, N)
    return o.download().reshape(len(moduli_out), N).T.tolist()


def crt_garner(residues, moduli, eng: Optional[Engine] = None):
    """``crt_kernel`` of rfhe_framewk/src/baseConv.cu:85-120; returns (x_lo, x_hi) arrays."""
    eng = eng or default_engine()
    r = _arr(residues)
    m, N = r.shape
    mod = _arr(moduli)
    d = eng.upload(r)
    lo, hi = eng.alloc(N), eng.alloc(N)
    check(lib.fhe_crt_garner(eng._h, lo.ptr, hi.ptr, d.ptr, _ptr(mod), m, N, None))
    return lo.download(), hi.download()


def diag_block_hadamard_matvec(M_blocks, v, mod: int = 0, eng: Optional[Engine] = None) -> np.ndarray:
    """``diag_block_hadamard_matvec`` of motivation/bsgs.py:39-52 (``mod=0``: the reference's
    unreduced int64 arithmetic)."""
    eng = eng or default_engine()
    M = np.ascontiguousarray(np.asarray(M_blocks, dtype=np.int64)).view(_U64)
    vv = np.ascontiguousarray(np.asarray(v, dtype=np.int64)).view(_U64)
    k, bs = M.shape
    dM, dv = eng.upload(M), eng.upload(vv)
    y = eng.alloc(k * bs)
    check(lib.fhe_bsgs_hadamard(eng._h, y.ptr, dM.ptr, dv.ptr, k, bs, mod, None))
    out = y.download()
    return out.view(np.int64) if mod == 0 else out


# ---------------------------------------------------------------------------
# Rotation / key switching
# ---------------------------------------------------------------------------
def automorphism(eng: Engine, t: NttTables, src: DeviceArray, galois_elt: int, n_poly: int = 1, limbs: Optional[int] = None,
                 start: int = 0, ntt_domain: bool = False) -> DeviceArray:
    """x -> x^galois_elt on every limb (coefficient domain, or NTT domain when ``ntt_domain``)."""
    limbs = len(t) - start if limbs is None else limbs
    dst = eng.alloc(src.size)
    dst.shape = src.shape
    if ntt_domain:
        check(lib.fhe_automorphism_ntt(eng._h, dst.ptr, src.ptr, t.log_n, galois_elt, n_poly * limbs, None))
    else:
        check(lib.fhe_automorphism(eng._h, dst.ptr, src.ptr, t._h, galois_elt, n_poly, limbs, start, None))
    return dst


def _permute_checked(eng: Engine, dst: DeviceArray, src: DeviceArray, log_n: int, galois_elt: int, units: int, stream=None) -> np.ndarray:
    return _checked_flags(eng, units, lambda fl: lib.fhe_automorphism_ntt_checked(eng._h, dst.ptr, src.ptr, log_n, galois_elt, units, fl.ptr, stream), stream)


def automorphism_checked(eng: Engine, t: NttTables, src: DeviceArray, galois_elt: int, n_poly: int = 1, limbs: Optional[int] = None):
    """``automorphism(..., ntt_domain=True)`` with one check per unit (row of N words): ``(dst, flags[n_units])``.  The words
    are the unchecked call's; flags[u] = 1 when the position-weighted sums of what row u read and of what it stored differ
    modulo 2^32 - 1: every single-bit flip of a moved word, and a wrong source index on all but about N / 2^32 of random words."""
    limbs = len(t) if limbs is None else limbs
    dst = eng.alloc(src.size)
    dst.shape = src.shape
    return dst, _permute_checked(eng, dst, src, t.log_n, galois_elt, n_poly * limbs)


def automorphism_sealed(eng: Engine, t: NttTables, src: DeviceArray, seal_src: DeviceArray, galois_elt: int, n_poly: int = 1,
                        limbs: Optional[int] = None, seal_out: bool = True, start: int = 0, stream=None):
    """``automorphism(..., ntt_domain=True)`` with the source's seal verified on the permutation's own gather: ``(dst, seal_dst,
    flags)``.  Each source word is loaded once, and the register that is stored is the register that is digested -- with its source
    weight against ``seal_src`` (from ``NttTables.seal``), with its destination weight for ``seal_dst`` (None when ``seal_out`` is
    false).  flags[poly * limbs + l] (uint32) carry ``seal_verify``'s bits: ``SEAL_SUM`` (1) the row as gathered is not the row
    that was sealed, ``SEAL_RANGE`` (2) a word >= q_l.  ``seal_dst`` is {S0 as stored in ``seal_src``, the digested S1}: a row whose
    S0 moved on this load keeps failing every later verification of ``dst``.  Not covered: a source change that keeps S0 and moves
    S1 alone raises the flag here but does not poison ``seal_dst`` (galois_seal.hpp)."""
    limbs = len(t) - start if limbs is None else limbs
    rows = n_poly * limbs
    dst = eng.alloc(src.size)
    dst.shape = src.shape
    seal_dst = None
    if seal_out:
        seal_dst = eng.alloc(rows * 2)
        seal_dst.shape = (rows, 2)
    flags = _checked_flags(eng, rows, lambda fl: lib.fhe_automorphism_ntt_sealed(
        eng._h, dst.ptr, src.ptr, seal_dst.ptr if seal_dst is not None else None, seal_src.ptr if seal_src is not None else None, t._h, n_poly, limbs, start,
        galois_elt, fl.ptr, stream), stream)
    return dst, seal_dst, flags


class KeySwitch:
    """Hybrid RNS key switching over the primes of ``t`` (L ciphertext primes then K special primes,
    ``dnum`` digits); operation sequence of the reference's SEAL trace
    (profile_framewk/build/data/ckks/16384_4:466-539)."""

    def __init__(self, eng: Engine, t: NttTables, L: int, K: int, dnum: int):
        self.eng, self.t, self.L, self.K, self.dnum = eng, t, L, K, dnum
        self.plain_modulus = 0
        h = vp()
        check(lib.fhe_keyswitch_create(eng._h, t._h, L, K, dnum, C.byref(h)))
        self._h = h

    def apply(self, c: DeviceArray, evk: DeviceArray, stream=None):
        """c: [L][N] NTT domain; evk: [dnum][2][L+K][N] NTT domain -> (out0, out1), each [L][N] NTT domain."""
        n = self.L * self.t.N
        o0, o1 = self.eng.alloc(n), self.eng.alloc(n)
        o0.shape = o1.shape = (self.L, self.t.N)
        check(lib.fhe_keyswitch_apply(self.eng._h, self._h, o0.ptr, o1.ptr, c.ptr, evk.ptr, stream))
        return o0, o1

    def rotate(self, c0: DeviceArray, c1: DeviceArray, galois_elt: int, galois_key: DeviceArray, stream=None):
        """``rotate_inplace`` (dotprod_test.cu:146) / frontend ROTATE of the SEAL traces: (c0, c1) -> (out0, out1)."""
        n = self.L * self.t.N
        o0, o1 = self.eng.alloc(n), self.eng.alloc(n)
        o0.shape = o1.shape = (self.L, self.t.N)
        check(lib.fhe_rotate(self.eng._h, self._h, o0.ptr, o1.ptr, c0.ptr, c1.ptr, galois_elt, galois_key.ptr, stream))
        return o0, o1

    def prepare_galois_key(self, galois_key: DeviceArray, galois_elt: int, stream=None) -> DeviceArray:
        """The key in the un-rotated frame (sigma^-1 of every key row): what ``rotate_hoisted`` takes; once per key."""
        out = self.eng.alloc(self.dnum * 2 * (self.L + self.K) * self.t.N)
        out.shape = (self.dnum, 2, self.L + self.K, self.t.N)
        check(lib.fhe_galois_key_prepare(self.eng._h, self._h, out.ptr, galois_key.ptr, galois_elt, stream))
        return out

    def rotate_hoisted(self, c0: DeviceArray, c1: DeviceArray, galois_elts, prepared_keys, stream=None):
        """Rotations of ONE ciphertext by several Galois elements with the decomposition of c1 shared (the baby steps of
        profile_framewk/src/matmul_ckks.cpp:45-113): a list of (out0, out1)."""
        n = len(galois_elts)
        outs = []
        for _ in range(n):
            o0, o1 = self.eng.alloc(self.L * self.t.N), self.eng.alloc(self.L * self.t.N)
            o0.shape = o1.shape = (self.L, self.t.N)
            outs.append((o0, o1))
        a0 = (vp * n)(*[o[0].ptr for o in outs])
        a1 = (vp * n)(*[o[1].ptr for o in outs])
        ks = (vp * n)(*[k.ptr for k in prepared_keys])
        ge = (C.c_uint32 * n)(*[int(g) for g in galois_elts])
        check(lib.fhe_rotate_hoisted(self.eng._h, self._h, a0, a1, c0.ptr, c1.ptr, ge, ks, n, stream))
        return outs

    def bsgs_matvec(self, c0: DeviceArray, c1: DeviceArray, diags: DeviceArray, n1: int, n2: int, baby_elts, baby_keys_prepared,
                    giant_elts, giant_keys, stream=None):
        """Baby-step / giant-step matrix-vector product (profile_framewk/src/matmul_ckks.cpp:45-113): diags = [n2][n1][L][N]."""
        o0, o1 = self._out(self.L), self._out(self.L)
        be = (C.c_uint32 * max(1, n1 - 1))(*[int(g) for g in baby_elts])
        ge = (C.c_uint32 * max(1, n2 - 1))(*[int(g) for g in giant_elts])
        bk = (vp * max(1, n1 - 1))(*[k.ptr for k in baby_keys_prepared])
        gk = (vp * max(1, n2 - 1))(*[k.ptr for k in giant_keys])
        check(lib.fhe_bsgs_matvec(self.eng._h, self._h, o0.ptr, o1.ptr, c0.ptr, c1.ptr, diags.ptr, n1, n2, be, bk, ge, gk, stream))
        return o0, o1

    def set_plain_modulus(self, t: int):
        """BGV form of the mod-down and of the rescale (0 = CKKS-style flooring)."""
        check(lib.fhe_keyswitch_set_plain_modulus(self._h, t))
        self.plain_modulus = int(t)

    def set_rescale_rounding(self, nearest: bool):
        """Rounding of every rescale on this plan (``rescale``, ``hmult`` with rescale): round to nearest -- SEAL's
        ``rescale_to_next_inplace``, floor((C + (q-1)/2) / q) -- instead of the default floor.  The checked and sealed calls that
        drop a prime refuse a plan that rounds to nearest; a plan with a plain modulus cannot round."""
        check(lib.fhe_keyswitch_set_rescale_rounding(self._h, 1 if nearest else 0))

    @property
    def rescale_rounding(self) -> bool:
        mode = C.c_int()
        check(lib.fhe_keyswitch_get_rescale_rounding(self._h, C.byref(mode)))
        return bool(mode.value)

    def _out(self, limbs: int) -> DeviceArray:
        o = self.eng.alloc(limbs * self.t.N)
        o.shape = (limbs, self.t.N)
        return o

    def tensor(self, a0: DeviceArray, a1: DeviceArray, b0: DeviceArray, b1: DeviceArray, stream=None):
        """``phantom::multiply`` (dotprod_test.cu:113): (d0, d1, d2), each [L][N], NTT domain."""
        d = [self._out(self.L) for _ in range(3)]
        check(lib.fhe_tensor_product(self.eng._h, d[0].ptr, d[1].ptr, d[2].ptr, a0.ptr, a1.ptr, b0.ptr, b1.ptr, self.t._h, self.L, 0, stream))
        return tuple(d)

    def tensor_checked(self, a0: DeviceArray, a1: DeviceArray, b0: DeviceArray, b1: DeviceArray, stream=None):
        """``tensor`` with every word checked: (d0, d1, d2, flags[L, 3]), flags[l, part] for d0 / d1 / d2 with the bits of
        ``NttTables.modmul_checked``.  The words are ``tensor``'s, bit for bit (FP64 terms on limbs below 2^50, Barrett above);
        the residue identity covers the lazy cross term d1 = a0 b1 + a1 b0 as one sum, the reference's Sum check
        (rfhe_framewk/src/barrett_final.py) and the element-wise fold check of four_step_ntt_protected.py:102-120."""
        d = [self._out(self.L) for _ in range(3)]
        f = _checked_flags(self.eng, 3 * self.L, lambda fl: lib.fhe_tensor_product_checked(
            self.eng._h, d[0].ptr, d[1].ptr, d[2].ptr, a0.ptr, a1.ptr, b0.ptr, b1.ptr, self.t._h, self.L, 0, fl.ptr, stream), stream)
        return d[0], d[1], d[2], f.reshape(self.L, 3)

    def relinearize(self, d0: DeviceArray, d1: DeviceArray, d2: DeviceArray, relin_key: DeviceArray, stream=None):
        """``relinearize_inplace`` (dotprod_test.cu:114)."""
        o0, o1 = self._out(self.L), self._out(self.L)
        check(lib.fhe_relinearize(self.eng._h, self._h, o0.ptr, o1.ptr, d0.ptr, d1.ptr, d2.ptr, relin_key.ptr, stream))
        return o0, o1

    # ---- stage-by-stage checked forms (capi_keyswitch_checked.cpp) ----
    CHECKED_STAGES = ("intt_in", "extend", "ntt_ext", "mac", "intt_special", "moddown", "ntt_conv", "tail")

    def checked_layout(self):
        """``{stage name: (offset, shape)}`` of the checked calls' flag words plus ``"total"``; M = L + K.  Stage names in order:
        ``intt_in [L]``, ``extend [dnum][M]``, ``ntt_ext [dnum][M]``, ``mac [2][M]``, ``intt_special [2][K]``,
        ``moddown [2][K + L]``, ``ntt_conv [2][L]``, ``tail [2][L]``."""
        return self._ks_layout(False)

    # Each checked composite below exists once, with its form as a parameter (bgv = False: the CKKS form, True: the BGV form of a
    # plan with a plain modulus); the public methods choose the form.
    @staticmethod
    def _c(bgv, name):
        """The C call ``name`` of a form: ``fhe_<name>``, or ``fhe_bgv_<name>`` with the rescale called mod_switch."""
        return getattr(lib, "fhe_bgv_" + name.replace("rescale", "mod_switch") if bgv else "fhe_" + name)

    def _ks_layout(self, bgv):
        names = self.BGV_CHECKED_STAGES if bgv else self.CHECKED_STAGES
        out = (C.c_int * 12)()
        check(self._c(bgv, "keyswitch_checked_layout")(self._h, out))
        L, K, d = self.L, self.K, self.dnum
        M = L + K
        shapes = ((L,), (d, M), (d, M), (2, M), (2, K), (2, K + L), (2, L), (2, L), (2, K), (2, L))
        lay = {name: (int(out[s]), shapes[s]) for s, name in enumerate(names)}
        lay["total"] = int(out[len(names)])
        return lay

    def _checked(self, bgv, name, *args, stream=None):
        """Run the key-switch call ``name`` of a form on (out0, out1, *args, flags): (out0, out1, flags by stage name)."""
        lay = self._ks_layout(bgv)
        o0, o1 = self._out(self.L), self._out(self.L)
        f = _checked_flags(self.eng, lay["total"], lambda fl: self._c(bgv, name)(self.eng._h, self._h, o0.ptr, o1.ptr, *args, fl.ptr, stream), stream)
        return o0, o1, self._split_flags(f, lay)

    def _apply_checked(self, bgv, c, evk, abft, add0, add1, stream):
        return self._checked(bgv, "keyswitch_apply_checked", c.ptr, evk.ptr, add0.ptr if add0 is not None else None,
                             add1.ptr if add1 is not None else None, abft._h, stream=stream)

    def _relinearize_checked(self, bgv, d0, d1, d2, relin_key, abft, stream):
        return self._checked(bgv, "relinearize_checked", d0.ptr, d1.ptr, d2.ptr, relin_key.ptr, abft._h, stream=stream)

    def _rotate_checked(self, bgv, c0, c1, galois_elt, galois_key, abft, stream):
        return self._checked(bgv, "rotate_checked", c0.ptr, c1.ptr, galois_elt, galois_key.ptr, abft._h, stream=stream)

    def apply_checked(self, c: DeviceArray, evk: DeviceArray, abft: "Abft", add0: Optional[DeviceArray] = None,
                      add1: Optional[DeviceArray] = None, stream=None):
        """``apply`` (plus the optional addends ``add0`` / ``add1``, [L][N]) with every stage checked: (out0, out1, flags).  The words
        are ``apply``'s bit for bit; ``flags`` maps each stage name of ``checked_layout`` to a uint32 array of its shape -- the ABFT
        stages hold 0 / 1, the residue-checked ones the bits 1 (identity), 2 (window), 4 (operand not canonical).  A fault at
        (stage, unit) raises that word and no other.  ``abft`` must be an ``Abft`` over the plan's tables."""
        return self._apply_checked(False, c, evk, abft, add0, add1, stream)

    def relinearize_checked(self, d0: DeviceArray, d1: DeviceArray, d2: DeviceArray, relin_key: DeviceArray, abft: "Abft", stream=None):
        """``relinearize`` with every stage of its key switch checked: (out0, out1, flags) as ``apply_checked``."""
        return self._relinearize_checked(False, d0, d1, d2, relin_key, abft, stream)

    def rotate_checked(self, c0: DeviceArray, c1: DeviceArray, galois_elt: int, galois_key: DeviceArray, abft: "Abft", stream=None):
        """``rotate`` with every stage of its key switch checked: (out0, out1, flags) as ``apply_checked``.  The Galois permutation
        of the two parts runs as a launch of its own and is not covered."""
        return self._rotate_checked(False, c0, c1, galois_elt, galois_key, abft, stream)

    # ---- checked hoisted rotations (capi_rotate_hoisted_checked.cpp) ----
    HOISTED_ROT_STAGES = ("mac", "galois", "intt_special", "moddown", "ntt_conv", "tail")      # in execution order

    def prepare_galois_key_checked(self, galois_key: DeviceArray, galois_elt: int, stream=None):
        """``prepare_galois_key`` through the checked permutation: ``(key, flags[dnum, 2, M])``, one word per key row."""
        M = self.L + self.K
        out = self.eng.alloc(self.dnum * 2 * M * self.t.N)
        out.shape = (self.dnum, 2, M, self.t.N)
        kinv = pow(int(galois_elt), -1, 2 * self.t.N)
        f = _permute_checked(self.eng, out, galois_key, self.t.log_n, kinv, self.dnum * 2 * M, stream)
        return out, f.reshape(self.dnum, 2, M)

    def rotate_hoisted_checked_layout(self, n_rot: int):
        """``{"shared": {stage: (offset, shape)}, "rot": {stage: (offset inside a rotation's block, shape)}, "shared_words",
        "rot_words", "total"}``; rotation r's block starts at ``shared_words + r * rot_words``.  Shared stages: ``intt_in [L]``,
        ``extend [dnum][M]``, ``ntt_ext [dnum][M]``; per rotation, in execution order: ``mac [2][M]``, ``galois [2 M + L]`` (the sums'
        rows half * M + row, then c0's rows), ``intt_special [2][K]``, ``moddown [2][K + L]``, ``ntt_conv [2][L]``, ``tail [2][L]``."""
        out = (C.c_int * 12)()
        check(lib.fhe_rotate_hoisted_checked_layout(self._h, n_rot, out))
        L, K, d = self.L, self.K, self.dnum
        M = L + K
        shared = ((L,), (d, M), (d, M))
        rot = ((2, M), (2 * M + L,), (2, K), (2, K + L), (2, L), (2, L))
        return {"shared": {name: (int(out[s]), shared[s]) for s, name in enumerate(self.CHECKED_STAGES[:3])},
                "rot": {name: (int(out[3 + i]), rot[i]) for i, name in enumerate(self.HOISTED_ROT_STAGES)},
                "shared_words": int(out[9]), "rot_words": int(out[10]), "total": int(out[11])}

    def rotate_hoisted_checked(self, c0: DeviceArray, c1: DeviceArray, galois_elts, prepared_keys, abft: "Abft", stream=None):
        """``rotate_hoisted`` with every stage checked, the Galois permutation included: ``(outs, flags)``.  ``outs`` is a list of
        (out0, out1) with ``rotate_hoisted``'s words bit for bit; ``flags = {"shared": {intt_in, extend, ntt_ext}, "rot": [{mac,
        galois, intt_special, moddown, ntt_conv, tail}, ...]}`` as ``rotate_hoisted_checked_layout`` shapes them.  The shared stages
        run once on the un-rotated c1; a fault there reaches every rotation, a fault in rotation r only its own words."""
        n = len(galois_elts)
        total = self.rotate_hoisted_checked_layout(n)["total"]
        outs = [(self._out(self.L), self._out(self.L)) for _ in range(n)]
        a0 = (vp * max(1, n))(*[o[0].ptr for o in outs])
        a1 = (vp * max(1, n))(*[o[1].ptr for o in outs])
        ks = (vp * max(1, n))(*[k.ptr for k in prepared_keys])
        ge = (C.c_uint32 * max(1, n))(*[int(g) for g in galois_elts])
        f = _checked_flags(self.eng, total, lambda fl: lib.fhe_rotate_hoisted_checked(self.eng._h, self._h, a0, a1, c0.ptr, c1.ptr, ge, ks, n, abft._h, fl.ptr,
                                                                                     stream), stream)
        return outs, self._hoisted_flags(f, n)

    def _hoisted_flags(self, f, n_rot, base=0):
        """The flag dictionary of ``n_rot`` checked hoisted rotations whose words start at ``f[base]``."""
        lay = self.rotate_hoisted_checked_layout(n_rot)
        return {"shared": self._split_flags(f, lay["shared"], lay["shared"], base),
                "rot": [self._split_flags(f, lay["rot"], lay["rot"], base + lay["shared_words"] + r * lay["rot_words"]) for r in range(n_rot)]}

    # ---- sealed hoisted rotations (capi_galois_sealed.cpp) ----
    def rotate_hoisted_sealed_layout(self, n_rot: int):
        """``{"c1": (0, (L,)), "rot0": offset of rotation 0's input block, "rot_words": words per rotation input block, "c0": (offset
        inside a rotation's input block, (L,)), "key": (offset inside it, (dnum, 2, M)), "checked": offset of the block laid out as
        rotate_hoisted_checked_layout, "total": n, "fused": the keys are verified on the inner product's load}`` of
        ``rotate_hoisted_sealed``'s flag buffer; rotation r's input block starts at ``rot0 + r * rot_words``."""
        out = (C.c_int * 6)()
        check(lib.fhe_rotate_hoisted_sealed_layout(self._h, n_rot, out))
        L, M = self.L, self.L + self.K
        return {"c1": (int(out[0]), (L,)), "rot0": int(out[1]), "rot_words": int(out[2]), "c0": (0, (L,)), "key": (L, (self.dnum, 2, M)),
                "checked": int(out[3]), "total": int(out[4]), "fused": bool(out[5])}

    def rotate_hoisted_sealed(self, c0: DeviceArray, c1: DeviceArray, galois_elts, prepared_keys, abft: "Abft", seals=None, key_seals=None,
                              seal_outputs: bool = True, stream=None):
        """``rotate_hoisted_checked`` with the operands protected at rest: ``(outs, out_seals, flags)``.  ``seals`` = the seals of
        (c0, c1) (either may be None), ``key_seals`` = one ``seal_key`` of each PREPARED key (entries may be None); ``out_seals`` is a
        list of (seal0, seal1), None entries when ``seal_outputs`` is false.  ``flags = {"c1": [L], "rot_in": [{"c0": [L], "key":
        [dnum][2][M]}, ...], "checked": <as rotate_hoisted_checked>}``.

        Each prepared key is verified on the inner product's own load (above 12 digits: by a sweep), and with c0's seal EVERY
        rotation verifies c0 on the gather of its own permutation: no sweep over c0 exists, and the c0 words of
        ``checked["rot"][r]["galois"]`` stay zero.  Without c0's seal c0 goes through the checked permutation as before.  c1 is swept
        once: its consuming load is inside the transform kernels.  Not covered on the consuming load: c1, sigma(c0) (re-read by the
        tail), the sums; no BGV, sharded or repairing form."""
        n = len(galois_elts)
        lay = self.rotate_hoisted_sealed_layout(n)
        outs = [(self._out(self.L), self._out(self.L)) for _ in range(n)]

        def seal_buf():
            s = self.eng.alloc(self.L * 2)
            s.shape = (self.L, 2)
            return s
        out_seals = [(seal_buf(), seal_buf()) if seal_outputs else (None, None) for _ in range(n)]
        m = max(1, n)
        ptr = lambda x: x.ptr if x is not None else None
        a0 = (vp * m)(*[o[0].ptr for o in outs])
        a1 = (vp * m)(*[o[1].ptr for o in outs])
        ks = (vp * m)(*[k.ptr for k in prepared_keys])
        ge = (C.c_uint32 * m)(*[int(g) for g in galois_elts])
        sin = (vp * 2)(*[ptr(x) for x in (seals if seals is not None else (None, None))])
        sk = (vp * m)(*[ptr(x) for x in (key_seals if key_seals is not None else [None] * n)])
        s0 = (vp * m)(*[ptr(x[0]) for x in out_seals])
        s1 = (vp * m)(*[ptr(x[1]) for x in out_seals])
        f = _checked_flags(self.eng, lay["total"], lambda fl: lib.fhe_rotate_hoisted_sealed(
            self.eng._h, self._h, a0, a1, c0.ptr, c1.ptr, ge, ks, n, abft._h, sin, sk, s0, s1, fl.ptr, stream), stream)
        flags = {"c1": self._split_flags(f, lay, ("c1",))["c1"],
                 "rot_in": [self._split_flags(f, lay, ("c0", "key"), lay["rot0"] + r * lay["rot_words"]) for r in range(n)],
                 "checked": self._hoisted_flags(f, n, lay["checked"])}
        return outs, out_seals, flags

    # ---- checked BSGS matrix-vector product (capi_bsgs_checked.cpp) ----
    BSGS_GIANT_STAGES = ("inner", "galois", "acc", "keyswitch")      # in execution order

    def bsgs_matvec_checked_layout(self, n1: int, n2: int):
        """``{"baby": 0, "baby_words", "giant0", "giant_words", "giant": {stage: (offset inside a giant block, shape)}, "total"}``.  The
        baby block is laid out as ``rotate_hoisted_checked_layout(n1 - 1)`` (no words when n1 == 1); giant block g starts at
        ``giant0 + g * giant_words`` and holds ``inner [2][L]``, ``galois [2 L]``, ``acc [L]`` and the key-switch block of
        ``checked_layout`` (for g = 0 only ``inner`` runs, the other words stay 0)."""
        out = (C.c_int * 8)()
        check(lib.fhe_bsgs_matvec_checked_layout(self._h, n1, n2, out))
        L = self.L
        shapes = ((2, L), (2 * L,), (L,), (self.checked_layout()["total"],))
        return {"baby": int(out[0]), "baby_words": int(out[1]), "giant0": int(out[1]), "giant_words": int(out[2]),
                "giant": {name: (int(out[3 + i]), shapes[i]) for i, name in enumerate(self.BSGS_GIANT_STAGES)}, "total": int(out[7])}

    def bsgs_matvec_checked(self, c0: DeviceArray, c1: DeviceArray, diags: DeviceArray, n1: int, n2: int, baby_elts, baby_keys_prepared,
                            giant_elts, giant_keys, abft: "Abft", stream=None):
        """``bsgs_matvec`` with every stage checked: ``(o0, o1, flags)``, the words ``bsgs_matvec``'s bit for bit.  ``flags = {"baby":
        <as rotate_hoisted_checked> or None when n1 == 1, "giant": [{"inner": [2][L], "galois": [2 L], "acc": [L], "keyswitch": {the
        eight stage names of checked_layout}}, ...]}``, one entry per giant step (for g = 0 only ``inner`` runs).  A fault raises the
        word of the (block, stage, unit) it hit and no other."""
        lay = self.bsgs_matvec_checked_layout(n1, n2)
        total = lay["total"]
        o0, o1 = self._out(self.L), self._out(self.L)
        be = (C.c_uint32 * max(1, n1 - 1))(*[int(g) for g in baby_elts])
        ge = (C.c_uint32 * max(1, n2 - 1))(*[int(g) for g in giant_elts])
        bk = (vp * max(1, n1 - 1))(*[k.ptr for k in baby_keys_prepared])
        gk = (vp * max(1, n2 - 1))(*[k.ptr for k in giant_keys])
        f = _checked_flags(self.eng, total, lambda fl: lib.fhe_bsgs_matvec_checked(
            self.eng._h, self._h, o0.ptr, o1.ptr, c0.ptr, c1.ptr, diags.ptr, n1, n2, be, bk, ge, gk, abft._h, fl.ptr, stream), stream)
        return o0, o1, self._bsgs_checked_flags(f, n1, n2)

    def rescale(self, c: DeviceArray, n_parts: int = 2, stream=None) -> DeviceArray:
        """``mod_switch_to_next_inplace`` (dotprod_test.cu:115): [n_parts][L][N] -> [n_parts][L-1][N]."""
        o = self.eng.alloc(n_parts * (self.L - 1) * self.t.N)
        o.shape = (n_parts, self.L - 1, self.t.N)
        check(lib.fhe_rescale(self.eng._h, self._h, o.ptr, c.ptr, n_parts, stream))
        return o

    def hmult(self, a0: DeviceArray, a1: DeviceArray, b0: DeviceArray, b1: DeviceArray, relin_key: DeviceArray, rescale: bool = True,
              stream=None):
        """multiply -> relinearize -> mod_switch_to_next (dotprod_test.cu:113-115) in one call."""
        limbs = self.L - 1 if rescale else self.L
        o0, o1 = self._out(limbs), self._out(limbs)
        check(lib.fhe_hmult(self.eng._h, self._h, o0.ptr, o1.ptr, a0.ptr, a1.ptr, b0.ptr, b1.ptr, relin_key.ptr, 1 if rescale else 0, stream))
        return o0, o1

    # ---- stage-by-stage checked rescale and homomorphic multiply (capi_hmult_checked.cpp) ----
    RESCALE_CHECKED_STAGES = ("intt_last", "reduce", "ntt_delta", "scale")

    def rescale_checked_layout(self, n_parts: int = 2):
        """``{stage name: (offset, shape)}`` of ``rescale_checked``'s flag words plus ``"total"``; R = L - 1.  Stage names in
        order: ``intt_last [n_parts]``, ``reduce [n_parts][R]``, ``ntt_delta [n_parts][R]``, ``scale [n_parts][R]``."""
        return self._rs_layout(False, n_parts)

    def hmult_checked_layout(self, rescale: bool = True):
        """``{"tensor": off, "keyswitch": off, "rescale": off, "total": n}`` of ``hmult_checked``'s flag buffer: the tensor block
        ``[L][3]``, the key-switch block laid out as ``checked_layout``, the rescale block as ``rescale_checked_layout(2)`` (its
        offset equals the total when ``rescale`` is false)."""
        return self._hm_layout(False, rescale)

    @staticmethod
    def _split_flags(f, lay, names=None, base=0):
        """The flag words of the stages ``names`` of a layout (default: all of them) as arrays of their shapes."""
        names = [n for n in lay if n != "total"] if names is None else names
        return {name: f[base + lay[name][0]:base + lay[name][0] + int(np.prod(lay[name][1]))].reshape(lay[name][1]).copy() for name in names}

    def _rs_layout(self, bgv, n_parts):
        names = self.BGV_MOD_SWITCH_CHECKED_STAGES if bgv else self.RESCALE_CHECKED_STAGES
        out = (C.c_int * 8)()
        check(self._c(bgv, "rescale_checked_layout")(self._h, n_parts, out))
        R = self.L - 1
        shapes = ((n_parts,), (n_parts, R), (n_parts, R), (n_parts, R), (n_parts,), (n_parts, R))
        lay = {name: (int(out[s]), shapes[s]) for s, name in enumerate(names)}
        lay["total"] = int(out[len(names)])
        return lay

    def _hm_layout(self, bgv, rescale):
        out = (C.c_int * 4)()
        check(self._c(bgv, "hmult_checked_layout")(self._h, 1 if rescale else 0, out))
        return {"tensor": int(out[0]), "keyswitch": int(out[1]), "rescale": int(out[2]), "total": int(out[3])}

    def _rescale_checked(self, bgv, c, abft, n_parts, stream):
        lay = self._rs_layout(bgv, n_parts)
        o = self.eng.alloc(n_parts * (self.L - 1) * self.t.N)
        o.shape = (n_parts, self.L - 1, self.t.N)
        f = _checked_flags(self.eng, lay["total"], lambda fl: self._c(bgv, "rescale_checked")(
            self.eng._h, self._h, o.ptr, c.ptr, n_parts, abft._h, fl.ptr, stream), stream)
        return o, self._split_flags(f, lay)

    def _hmult_flags(self, bgv, f, rescale, base=0):
        """The flags of a form's checked multiply, whose block starts at word ``base`` of ``f``, by step and stage name."""
        lay, kl = self._hm_layout(bgv, rescale), self._ks_layout(bgv)
        rl = self._rs_layout(bgv, 2) if rescale else None
        t0 = base + lay["tensor"]
        return {"tensor": f[t0:t0 + 3 * self.L].reshape(self.L, 3).copy(),
                "keyswitch": self._split_flags(f, kl, base=base + lay["keyswitch"]),
                "rescale": self._split_flags(f, rl, base=base + lay["rescale"]) if rescale else None}

    def _hmult_checked(self, bgv, a0, a1, b0, b1, relin_key, abft, rescale, stream):
        limbs = self.L - 1 if rescale else self.L
        o0, o1 = self._out(limbs), self._out(limbs)
        f = _checked_flags(self.eng, self._hm_layout(bgv, rescale)["total"], lambda fl: self._c(bgv, "hmult_checked")(
            self.eng._h, self._h, o0.ptr, o1.ptr, a0.ptr, a1.ptr, b0.ptr, b1.ptr, relin_key.ptr, 1 if rescale else 0, abft._h, fl.ptr, stream), stream)
        return o0, o1, self._hmult_flags(bgv, f, rescale)

    def rescale_checked(self, c: DeviceArray, abft: "Abft", n_parts: int = 2, stream=None):
        """``rescale`` with every stage checked: (out, flags).  The words are ``rescale``'s bit for bit; ``flags`` maps
        ``intt_last``, ``reduce``, ``ntt_delta`` and ``scale`` to uint32 arrays of the shapes of ``rescale_checked_layout`` -- the ABFT
        stages hold 0 / 1, the residue-checked ones the bits 1 (identity), 2 (window), 4 (operand not canonical).  A fault at
        (stage, unit) raises that word and no other."""
        return self._rescale_checked(False, c, abft, n_parts, stream)

    def hmult_checked(self, a0: DeviceArray, a1: DeviceArray, b0: DeviceArray, b1: DeviceArray, relin_key: DeviceArray, abft: "Abft",
                      rescale: bool = True, stream=None):
        """``hmult`` with every step checked -- multiply -> relinearize -> mod_switch_to_next (dotprod_test.cu:113-115) as one
        protected call: (out0, out1, flags), the words ``hmult``'s bit for bit.  ``flags = {"tensor": [L][3] as tensor_checked,
        "keyswitch": {the eight stage names of checked_layout}, "rescale": {the four of rescale_checked_layout} or None}``."""
        return self._hmult_checked(False, a0, a1, b0, b1, relin_key, abft, rescale, stream)

    # ---- BGV forms of the checked calls: plans with a plain modulus ----
    BGV_CHECKED_STAGES = CHECKED_STAGES + ("scale_special", "scale_conv")                # stages 0-7, then 9 and 10
    BGV_MOD_SWITCH_CHECKED_STAGES = RESCALE_CHECKED_STAGES + ("scale_last", "scale_delta")   # stages 0-3, then 4 and 5

    def bgv_checked_layout(self):
        """``checked_layout`` of the BGV key switch: the eight stages at the same offsets, then ``scale_special [2][K]`` (stage 9: the
        special limbs times t^-1, run between ``intt_special`` and ``moddown``) and ``scale_conv [2][L]`` (stage 10: the converted
        limbs times t, run between ``moddown`` and ``ntt_conv``), plus ``"total"``."""
        return self._ks_layout(True)

    def bgv_apply_checked(self, c: DeviceArray, evk: DeviceArray, abft: "Abft", add0: Optional[DeviceArray] = None,
                          add1: Optional[DeviceArray] = None, stream=None):
        """``apply`` on a plan with a plain modulus with every stage checked, the two BGV scalar stages included: (out0, out1,
        flags) as ``apply_checked``, ``flags`` keyed by the ten names of ``bgv_checked_layout``."""
        return self._apply_checked(True, c, evk, abft, add0, add1, stream)

    def bgv_relinearize_checked(self, d0: DeviceArray, d1: DeviceArray, d2: DeviceArray, relin_key: DeviceArray, abft: "Abft", stream=None):
        """``relinearize`` on a BGV plan with every stage checked: (out0, out1, flags) as ``bgv_apply_checked``."""
        return self._relinearize_checked(True, d0, d1, d2, relin_key, abft, stream)

    def bgv_rotate_checked(self, c0: DeviceArray, c1: DeviceArray, galois_elt: int, galois_key: DeviceArray, abft: "Abft", stream=None):
        """``rotate`` on a BGV plan with every stage of its key switch checked: (out0, out1, flags) as ``bgv_apply_checked``.  The
        Galois permutation runs as a launch of its own and is not covered, as for ``rotate_checked``."""
        return self._rotate_checked(True, c0, c1, galois_elt, galois_key, abft, stream)

    def bgv_mod_switch_checked_layout(self, n_parts: int = 2):
        """``rescale_checked_layout`` of the BGV mod switch: the four stages at the same offsets, then ``scale_last [n_parts]``
        (stage 4: the last limbs times t^-1, run between ``intt_last`` and ``reduce``) and ``scale_delta [n_parts][R]`` (stage 5: the
        residues times t, run between ``reduce`` and ``ntt_delta``), plus ``"total"``."""
        return self._rs_layout(True, n_parts)

    def bgv_mod_switch_checked(self, c: DeviceArray, abft: "Abft", n_parts: int = 2, stream=None):
        """``rescale`` on a BGV plan (``mod_switch_to_next_inplace``, dotprod_test.cu:115) with every stage checked: (out, flags) as
        ``rescale_checked``, ``flags`` keyed by the six names of ``bgv_mod_switch_checked_layout``."""
        return self._rescale_checked(True, c, abft, n_parts, stream)

    def bgv_hmult_checked_layout(self, rescale: bool = True):
        """``hmult_checked_layout`` with the two BGV layouts: ``{"tensor": off, "keyswitch": off, "rescale": off, "total": n}``."""
        return self._hm_layout(True, rescale)

    def bgv_hmult_checked(self, a0: DeviceArray, a1: DeviceArray, b0: DeviceArray, b1: DeviceArray, relin_key: DeviceArray, abft: "Abft",
                          rescale: bool = True, stream=None):
        """``hmult`` on a BGV plan with every step checked -- the reference's multiply -> relinearize_inplace ->
        mod_switch_to_next_inplace (dotprod_test.cu:113-115) as one protected call: (out0, out1, flags) as ``hmult_checked``, the
        key-switch and mod-switch blocks keyed by the names of ``bgv_checked_layout`` / ``bgv_mod_switch_checked_layout``."""
        return self._hmult_checked(True, a0, a1, b0, b1, relin_key, abft, rescale, stream)

    # ---- operands sealed at rest: the checked multiply and rotation behind seal verification (capi_seal.cpp) ----
    def seal_key(self, key: DeviceArray, stream=None) -> DeviceArray:
        """The seal of a relinearisation or Galois key ``[dnum][2][L + K][N]``: ``[dnum * 2 * (L + K)][2]``."""
        return self.t.seal(key, limbs=self.L + self.K, start=0, n_poly=2 * self.dnum, stream=stream)

    def _sealed_layout(self, out, names, checked, total):
        L, M = self.L, self.L + self.K
        lay = {name: (int(out[i]), (L,)) for i, name in enumerate(names)}
        lay["key"] = (int(out[len(names)]), (self.dnum, 2, M))
        lay["checked"], lay["total"] = int(out[checked]), int(out[total])
        return lay

    def hmult_sealed_layout(self, rescale: bool = True):
        """``{"a0", "a1", "b0", "b1": (offset, (L,)), "key": (offset, (dnum, 2, M)), "checked": offset, "total": n}`` of
        ``hmult_sealed``'s flag buffer: the input rows in argument order, the key's rows, then the checked multiply's own block
        (``hmult_checked_layout``, or ``bgv_hmult_checked_layout`` on a plan with a plain modulus)."""
        out = (C.c_int * 8)()
        check(lib.fhe_hmult_sealed_layout(self._h, 1 if rescale else 0, out))
        return self._sealed_layout(out, ("a0", "a1", "b0", "b1"), 5, 6)

    def rotate_sealed_layout(self):
        """``{"c0", "c1": (offset, (L,)), "key": (offset, (dnum, 2, M)), "checked": offset, "total": n}`` of ``rotate_sealed``'s
        flag buffer; the checked block is laid out as ``checked_layout`` (``bgv_checked_layout`` with a plain modulus)."""
        out = (C.c_int * 6)()
        check(lib.fhe_rotate_sealed_layout(self._h, out))
        return self._sealed_layout(out, ("c0", "c1"), 3, 4)

    def _sealed(self, lay, names, limbs, seals, call, stream):
        """Run ``call(o0, o1, seal_in, seal_out, flags)``; returns (o0, o1, (seal0, seal1), flat flags)."""
        o0, o1 = self._out(limbs), self._out(limbs)
        so = [self.eng.alloc(2 * limbs) for _ in range(2)]
        for x in so:
            x.shape = (limbs, 2)
        seals = tuple(seals) if seals is not None else (None,) * len(names)
        sin = (vp * len(names))(*[x.ptr if x is not None else None for x in seals])
        sout = (vp * 2)(so[0].ptr, so[1].ptr)
        f = _checked_flags(self.eng, lay["total"], lambda fl: call(o0, o1, sin, sout, fl), stream)
        return o0, o1, tuple(so), f

    def hmult_sealed(self, a0: DeviceArray, a1: DeviceArray, b0: DeviceArray, b1: DeviceArray, relin_key: DeviceArray, abft: "Abft",
                     seals=None, key_seal: Optional[DeviceArray] = None, rescale: bool = True, stream=None):
        """``hmult_checked`` (``bgv_hmult_checked`` on a plan with a plain modulus) with the operands protected at rest: every given
        seal is verified, the checked multiply runs unchanged, both outputs are sealed: ``(out0, out1, (seal0, seal1), flags)``.
        ``seals`` = the seals of (a0, a1, b0, b1) from ``NttTables.seal`` (an entry, or all, may be None: not verified),
        ``key_seal`` from ``seal_key``.  ``flags = {"a0", "a1", "b0", "b1": [L], "key": [dnum][2][M], "checked": <the flags of the
        checked multiply>}``, input words with the bits of ``seal_verify``.  A raised input flag does not stop the call; the checked
        block and the output seals are then meaningless.  The words are ``hmult``'s, bit for bit."""
        return self._hmult_sealed(lib.fhe_hmult_sealed, a0, a1, b0, b1, relin_key, abft, seals, key_seal, rescale, stream)

    def _hmult_sealed(self, call, a0, a1, b0, b1, relin_key, abft, seals, key_seal, rescale, stream):
        names = ("a0", "a1", "b0", "b1")
        lay = self.hmult_sealed_layout(rescale)
        o0, o1, so, f = self._sealed(lay, names, self.L - 1 if rescale else self.L, seals, lambda o0, o1, sin, sout, fl: call(
            self.eng._h, self._h, o0.ptr, o1.ptr, a0.ptr, a1.ptr, b0.ptr, b1.ptr, relin_key.ptr, 1 if rescale else 0, abft._h, sin,
            key_seal.ptr if key_seal is not None else None, sout, fl.ptr, stream), stream)
        flags = self._split_flags(f, lay, names + ("key",))
        flags["checked"] = self._hmult_flags(bool(self.plain_modulus), f, rescale, lay["checked"])
        return o0, o1, so, flags

    # ---- sealed tensor product: the operands verified on the load that multiplies them (tensor_sealed.hip) ----
    def tensor_sealed_layout(self):
        """``{"a0", "a1", "b0", "b1": (offset, (L,)), "tensor": (offset, (L, 3)), "total": n}`` of ``tensor_sealed``'s flag buffer."""
        out = (C.c_int * 6)()
        check(lib.fhe_tensor_product_sealed_layout(1, self.L, out))
        lay = {name: (int(out[i]), (self.L,)) for i, name in enumerate(("a0", "a1", "b0", "b1"))}
        lay["tensor"], lay["total"] = (int(out[4]), (self.L, 3)), int(out[5])
        return lay

    def tensor_sealed(self, a0: DeviceArray, a1: DeviceArray, b0: DeviceArray, b1: DeviceArray, seals=None, seal_out: bool = True, stream=None):
        """``tensor_checked`` with the operands verified on the very load that multiplies them, and the results sealed from the
        registers that are stored: ``(d0, d1, d2, (s0, s1, s2) or None, flags)``.  ``seals`` = the seals of (a0, a1, b0, b1) from
        ``NttTables.seal`` (an entry, or all, may be None: not compared -- the window word < q_l is checked all the same);
        ``seal_out = False``: no result is digested.  ``flags = {"a0", "a1", "b0", "b1": [L], "tensor": [L, 3]}``: operand words
        with the bits of ``seal_verify``, the tensor block with those of ``tensor_checked``.  The words are ``tensor``'s, bit for
        bit, also for an operand word that is not canonical: it is flagged, not fixed.

        Covered: a change confined to one or two words of an operand row, at rest or on this call's own load, with certainty
        (seal_check.hpp); no operand word is read twice.  A changed operand raises its row and not the tensor block: the residue
        identity holds on the operand as loaded.  Not covered: a fault after the results' digest (the store, memory) -- whoever
        verifies (s0, s1, s2) next sees it; an output may be an operand's buffer, and a may be b."""
        names = ("a0", "a1", "b0", "b1")
        lay = self.tensor_sealed_layout()
        d = [self._out(self.L) for _ in range(3)]
        so = [self.eng.alloc(2 * self.L) for _ in range(3)] if seal_out else None
        for x in so or ():
            x.shape = (self.L, 2)
        seals = tuple(seals) if seals is not None else (None,) * 4
        sin = (vp * 4)(*[x.ptr if x is not None else None for x in seals])
        sout = (vp * 3)(*[x.ptr for x in so]) if seal_out else None
        f = _checked_flags(self.eng, lay["total"], lambda fl: lib.fhe_tensor_product_sealed(
            self.eng._h, d[0].ptr, d[1].ptr, d[2].ptr, a0.ptr, a1.ptr, b0.ptr, b1.ptr, self.t._h, 1, self.L, 0, sin, sout, fl.ptr, stream), stream)
        return d[0], d[1], d[2], tuple(so) if seal_out else None, self._split_flags(f, lay, names + ("tensor",))

    def hmult_sealed_fused(self, a0: DeviceArray, a1: DeviceArray, b0: DeviceArray, b1: DeviceArray, relin_key: DeviceArray, abft: "Abft",
                           seals=None, key_seal: Optional[DeviceArray] = None, rescale: bool = True, stream=None):
        """``hmult_sealed`` -- same arguments, same result structure, same words and flag layout -- without the four operand sweeps:
        the multiply's tensor step is ``tensor_sealed``'s kernel, so a0, a1, b0, b1 are verified on the load that multiplies them
        and a fault on that load raises the operand's row.  An operand without a seal is not compared, but its window is still
        checked.  Not covered on the consuming load: the key (verified by its sweep, loaded again by the key switch) and the
        plan's d0, d1, d2, which the key switch re-reads; no repairing form."""
        return self._hmult_sealed(lib.fhe_hmult_sealed_fused, a0, a1, b0, b1, relin_key, abft, seals, key_seal, rescale, stream)

    def rotate_sealed(self, c0: DeviceArray, c1: DeviceArray, galois_elt: int, galois_key: DeviceArray, abft: "Abft", seals=None,
                      key_seal: Optional[DeviceArray] = None, stream=None):
        """``rotate_checked`` (``bgv_rotate_checked`` on a plan with a plain modulus) with the operands protected at rest:
        ``(out0, out1, (seal0, seal1), flags)`` as ``hmult_sealed``; ``seals`` = the seals of (c0, c1), ``flags = {"c0", "c1": [L],
        "key": [dnum][2][M], "checked": {the stage names of checked_layout / bgv_checked_layout}}``."""
        return self._rotate_sealed(lib.fhe_rotate_sealed, c0, c1, galois_elt, galois_key, abft, seals, key_seal, stream)

    def _rotate_sealed(self, call, c0, c1, galois_elt, galois_key, abft, seals, key_seal, stream, lay=None, rows=("c0", "c1")):
        """One sealed rotation: ``lay`` its layout (``rotate_sealed_layout`` by default), ``rows`` the input blocks of its flags."""
        lay = lay or self.rotate_sealed_layout()
        o0, o1, so, f = self._sealed(lay, ("c0", "c1"), self.L, seals, lambda o0, o1, sin, sout, fl: call(
            self.eng._h, self._h, o0.ptr, o1.ptr, c0.ptr, c1.ptr, galois_elt, galois_key.ptr, abft._h, sin,
            key_seal.ptr if key_seal is not None else None, sout, fl.ptr, stream), stream)
        flags = self._split_flags(f, lay, rows + ("key",))
        flags["checked"] = self._split_flags(f, self._ks_layout(bool(self.plain_modulus)), base=lay["checked"])
        return o0, o1, so, flags

    # ---- sealed key-switch inner product: the key verified on the load that multiplies it (keyswitch_sealed.hip) ----
    def apply_sealed_layout(self):
        """``{"key": (offset, (dnum, 2, M)), "checked": offset, "total": n, "fused": bool}`` of ``apply_sealed``'s flag buffer; the
        checked block is laid out as ``checked_layout`` (``bgv_checked_layout`` with a plain modulus).  ``fused``: the plan's
        ``dnum`` has a fused instantiation (at most 12 digits); otherwise the key is swept before the checked inner product."""
        out = (C.c_int * 4)()
        check(lib.fhe_keyswitch_sealed_layout(self._h, out))
        return {"key": (int(out[0]), (self.dnum, 2, self.L + self.K)), "checked": int(out[1]), "total": int(out[2]), "fused": bool(out[3])}

    def apply_sealed(self, c: DeviceArray, evk: DeviceArray, abft: "Abft", key_seal: Optional[DeviceArray] = None,
                     add0: Optional[DeviceArray] = None, add1: Optional[DeviceArray] = None, stream=None):
        """``apply_checked`` (``bgv_apply_checked`` on a plan with a plain modulus) with the key verified on the very load that
        multiplies it: ``(out0, out1, flags)``, ``flags = {"key": [dnum][2][M], "checked": {the stage names of checked_layout /
        bgv_checked_layout}}``, key words with the bits of ``seal_verify``.  ``key_seal`` from ``seal_key`` (None: not compared --
        the window word < q_j is checked all the same).  The words are ``apply``'s, bit for bit, also for a key word that is not
        canonical: it is flagged, not fixed.

        Covered: a change confined to one or two words of a key row, at rest or on the inner product's own load, with certainty
        (seal_check.hpp); no key word is read twice.  A changed key word raises its row and not ``checked["mac"]``: the residue
        identity holds on the key as loaded.  Not covered on the consuming load: ``c`` (its loads are inside transform kernels)
        and the plan's digits, which the inner product also loads."""
        return self._apply_sealed(lib.fhe_keyswitch_apply_sealed, self.apply_sealed_layout(), ("key",), c, evk, abft, (key_seal,), add0, add1, stream)

    def _apply_sealed(self, call, lay, rows, c, evk, abft, seals, add0, add1, stream):
        """One sealed key switch: ``seals`` the seal arguments of ``call`` in its order, ``rows`` the input blocks of its flags."""
        o0, o1 = self._out(self.L), self._out(self.L)
        f = _checked_flags(self.eng, lay["total"], lambda fl: call(
            self.eng._h, self._h, o0.ptr, o1.ptr, c.ptr, evk.ptr, add0.ptr if add0 is not None else None, add1.ptr if add1 is not None else None,
            abft._h, *[x.ptr if x is not None else None for x in seals], fl.ptr, stream), stream)
        flags = self._split_flags(f, lay, rows)
        flags["checked"] = self._split_flags(f, self._ks_layout(bool(self.plain_modulus)), base=lay["checked"])
        return o0, o1, flags

    # ---- sealed inverse NTT: the input limbs verified on the opening transform's own load (ntt_sealed.hip) ----
    def apply_sealed_in_layout(self):
        """``{"c": (offset, (L,)), "key": (offset, (dnum, 2, M)), "checked": offset, "total": n, "fused": bool}`` of
        ``apply_sealed_in``'s flag buffer; the checked block is laid out as ``checked_layout`` (``bgv_checked_layout`` with a plain
        modulus)."""
        out = (C.c_int * 5)()
        check(lib.fhe_keyswitch_sealed_in_layout(self._h, out))
        return {"c": (int(out[0]), (self.L,)), "key": (int(out[1]), (self.dnum, 2, self.L + self.K)), "checked": int(out[2]), "total": int(out[3]),
                "fused": bool(out[4])}

    def apply_sealed_in(self, c: DeviceArray, evk: DeviceArray, abft: "Abft", c_seal: DeviceArray, key_seal: Optional[DeviceArray] = None,
                        add0: Optional[DeviceArray] = None, add1: Optional[DeviceArray] = None, stream=None):
        """``apply_sealed`` with the input limbs sealed as well: ``(out0, out1, flags)``, ``flags = {"c": [L], "key": [dnum][2][M],
        "checked": {...}}``.  Stage 0 makes no copy of ``c``: the opening inverse transform reads ``c`` itself, digests every word
        from the register its first step holds and is held against ``c_seal`` (from ``NttTables.seal``; required).  The words are
        ``apply``'s.  Not covered: the inner product's own load of ``c`` and of the plan's digits."""
        return self._apply_sealed(lib.fhe_keyswitch_apply_sealed_in, self.apply_sealed_in_layout(), ("c", "key"), c, evk, abft, (c_seal, key_seal), add0, add1,
                                  stream)

    def rotate_sealed_in_layout(self):
        """``{"c0", "c1", "sigma_c1": (offset, (L,)), "key": (offset, (dnum, 2, M)), "checked": offset, "total": n, "fused": bool}``
        of ``rotate_sealed_in``'s flag buffer."""
        out = (C.c_int * 7)()
        check(lib.fhe_rotate_sealed_in_layout(self._h, out))
        lay = {name: (int(out[i]), (self.L,)) for i, name in enumerate(("c0", "c1", "sigma_c1"))}
        lay.update({"key": (int(out[3]), (self.dnum, 2, self.L + self.K)), "checked": int(out[4]), "total": int(out[5]), "fused": bool(out[6])})
        return lay

    def rotate_sealed_in(self, c0: DeviceArray, c1: DeviceArray, galois_elt: int, galois_key: DeviceArray, abft: "Abft", seals,
                         key_seal: Optional[DeviceArray] = None, stream=None):
        """``rotate_sealed_fused`` without the sweeps over c0 and c1 and without the unchecked permutation: ``(out0, out1, (seal0,
        seal1), flags)``, ``flags = {"c0", "c1", "sigma_c1": [L], "key": [dnum][2][M], "checked": {...}}``.  c0 and c1 (``seals`` =
        their seals, both required) are verified on the sealed permutation's gather, sigma(c1)'s seal is written from the registers
        that are stored, and the opening inverse transform verifies sigma(c1) against it on its own load.  The words are
        ``rotate``'s.  Not covered: sigma(c0), which the tail re-reads from the plan; the inner product's own loads."""
        return self._rotate_sealed_in(lib.fhe_rotate_sealed_in, c0, c1, galois_elt, galois_key, abft, seals, key_seal, stream)

    def _rotate_sealed_in(self, call, c0, c1, galois_elt, galois_key, abft, seals, key_seal, stream):
        return self._rotate_sealed(call, c0, c1, galois_elt, galois_key, abft, seals, key_seal, stream, self.rotate_sealed_in_layout(),
                                   ("c0", "c1", "sigma_c1"))

    def rotate_sealed_fused(self, c0: DeviceArray, c1: DeviceArray, galois_elt: int, galois_key: DeviceArray, abft: "Abft", seals=None,
                            key_seal: Optional[DeviceArray] = None, stream=None):
        """``rotate_sealed`` -- same arguments, same result structure, same words and flag layout -- without the key's sweep: the key
        switch's inner product is ``apply_sealed``'s kernel, so the Galois key is verified on the load that multiplies it and a
        fault on that load raises the key's row.  The sweeps over c0 and c1 stay.  No repairing form."""
        return self._rotate_sealed(lib.fhe_rotate_sealed_fused, c0, c1, galois_elt, galois_key, abft, seals, key_seal, stream)

    def hmult_sealed_fused_key(self, a0: DeviceArray, a1: DeviceArray, b0: DeviceArray, b1: DeviceArray, relin_key: DeviceArray, abft: "Abft",
                               seals=None, key_seal: Optional[DeviceArray] = None, rescale: bool = True, stream=None):
        """``hmult_sealed_fused`` -- same arguments, same result structure, same words and flag layout -- with the relinearisation
        key fused as well: no input is swept at all.  Not covered on the consuming load: the plan's d0, d1, d2 and digits, which
        the key switch re-reads; no repairing form."""
        return self._hmult_sealed(lib.fhe_hmult_sealed_fused_key, a0, a1, b0, b1, relin_key, abft, seals, key_seal, rescale, stream)

    # ---- sealed rescale and sealed tail: inputs verified on load, outputs sealed on store (subscale_sealed.hip) ----
    def rescale_sealed_layout(self, n_parts: int = 2):
        """``{"in": (offset, (n_parts, L)), "checked": offset, "total": n}`` of ``rescale_sealed``'s flag buffer; the checked block is
        laid out as ``rescale_checked_layout`` (``bgv_mod_switch_checked_layout`` with a plain modulus)."""
        out = (C.c_int * 4)()
        check(lib.fhe_rescale_sealed_layout(self._h, n_parts, out))
        return {"in": (int(out[0]), (n_parts, self.L)), "checked": int(out[1]), "total": int(out[2])}

    def rescale_sealed(self, c: DeviceArray, abft: "Abft", seal: DeviceArray, n_parts: int = 2, stream=None):
        """``rescale_checked`` (``bgv_mod_switch_checked`` on a plan with a plain modulus) with the input verified on the loads that
        consume it and the output sealed from the registers that are stored: ``(out, seal_out, flags)``, ``seal`` = the input's
        seal ``[n_parts][L][2]`` from ``NttTables.seal`` (required), ``seal_out`` = ``[n_parts][L - 1][2]``, ``flags = {"in":
        [n_parts][L], "checked": {the stage names of rescale_checked_layout / bgv_mod_switch_checked_layout}}``, input words with
        the bits of ``seal_verify``.  No copy and no sweep: the last limbs are verified on the opening inverse transform's load, the
        other rows on the load that subtracts from them.  The words are ``rescale``'s, bit for bit.  Not covered: the plan's own
        residues, which the tail also loads; a fault after the output's digest -- whoever verifies ``seal_out`` next sees it."""
        lay = self.rescale_sealed_layout(n_parts)
        R = self.L - 1
        o = self.eng.alloc(n_parts * R * self.t.N)
        o.shape = (n_parts, R, self.t.N)
        so = self.eng.alloc(n_parts * R * 2)
        so.shape = (n_parts, R, 2)
        f = _checked_flags(self.eng, lay["total"], lambda fl: lib.fhe_rescale_sealed(
            self.eng._h, self._h, o.ptr, c.ptr, n_parts, abft._h, seal.ptr if seal is not None else None, so.ptr, fl.ptr, stream), stream)
        flags = self._split_flags(f, lay, ("in",))
        flags["checked"] = self._split_flags(f, self._rs_layout(bool(self.plain_modulus), n_parts), base=lay["checked"])
        return o, so, flags

    def hmult_sealed_out(self, a0: DeviceArray, a1: DeviceArray, b0: DeviceArray, b1: DeviceArray, relin_key: DeviceArray, abft: "Abft",
                         seals=None, key_seal: Optional[DeviceArray] = None, rescale: bool = True, stream=None):
        """``hmult_sealed_fused_key`` -- same arguments, same result structure, same words and flag layout -- without the two output
        sweeps: the multiply's last launch writes both outputs' seals from the registers it stores."""
        return self._hmult_sealed(lib.fhe_hmult_sealed_out, a0, a1, b0, b1, relin_key, abft, seals, key_seal, rescale, stream)

    def rotate_sealed_out(self, c0: DeviceArray, c1: DeviceArray, galois_elt: int, galois_key: DeviceArray, abft: "Abft", seals,
                          key_seal: Optional[DeviceArray] = None, stream=None):
        """``rotate_sealed_in`` -- same arguments, same result structure, same words and flag layout -- without the two output
        sweeps: the key switch's last launch writes both outputs' seals from the registers it stores."""
        return self._rotate_sealed_in(lib.fhe_rotate_sealed_out, c0, c1, galois_elt, galois_key, abft, seals, key_seal, stream)

    def rotate_sum_sealed_layout(self, n_steps: int):
        """``{"stride": words per step, "add": offset of the add rows inside a step's block, "total": n, "rotate": the layout of
        rotate_sealed_layout, which a step's block starts with}`` of ``rotate_sum_sealed``'s flag buffer."""
        out = (C.c_int * 4)()
        check(lib.fhe_rotate_sum_sealed_layout(self._h, n_steps, out))
        return {"stride": int(out[0]), "add": int(out[1]), "total": int(out[2]), "rotate": self.rotate_sealed_layout()}

    def rotate_sum_sealed(self, c0: DeviceArray, c1: DeviceArray, galois_elts: Sequence[int], galois_keys: Sequence[DeviceArray], abft: "Abft", seals,
                          key_seals=None, stream=None):
        """The tail of the reference's dot product (dotprod_test.cu:143-148: per step rotated = xy; rotate_inplace(rotated, step);
        add_inplace(xy, rotated)) as one protected call: per step ``rotate_sealed`` from the accumulators into a rotated copy, then
        one carried add per half back into them (``NttTables.modadd_sealed``), the seals updated in place.  Works on copies of
        (c0, c1) and of ``seals``: ``(out0, out1, (seal0, seal1), flags)`` with ``flags`` a list with one dictionary per step,
        ``rotate_sealed``'s plus ``"add0"``, ``"add1"``: [L] (the bits of ``modadd_sealed``).  ``key_seals``: one per step, entries
        or all may be None.  Every load in it is a verified load: step s + 1 verifies on entry what step s's adds stored."""
        n, L = len(galois_elts), self.L
        lay = self.rotate_sum_sealed_layout(n)
        acc, tmp = [self._out(L), self._out(L)], [self._out(L), self._out(L)]
        sl, st = [self.eng.alloc(2 * L) for _ in range(2)], [self.eng.alloc(2 * L) for _ in range(2)]
        for h, (src, seal) in enumerate(zip((c0, c1), seals)):
            acc[h].copy_from(src)
            sl[h].copy_from(seal)
            sl[h].shape = (L, 2)
        self.eng.sync()
        elts = (C.c_uint32 * n)(*galois_elts)
        keys = (vp * n)(*[k.ptr for k in galois_keys])
        ksl = (vp * n)(*[x.ptr if x is not None else None for x in key_seals]) if key_seals is not None else None
        f = _checked_flags(self.eng, lay["total"], lambda fl: lib.fhe_rotate_sum_sealed(
            self.eng._h, self._h, acc[0].ptr, acc[1].ptr, tmp[0].ptr, tmp[1].ptr, n, elts, keys, abft._h, (vp * 2)(sl[0].ptr, sl[1].ptr), ksl,
            (vp * 2)(st[0].ptr, st[1].ptr), fl.ptr, stream), stream)
        rl, kl = lay["rotate"], self._ks_layout(bool(self.plain_modulus))
        steps = []
        for s in range(n):
            base = s * lay["stride"]
            d = self._split_flags(f, rl, ("c0", "c1", "key"), base=base)
            d["checked"] = self._split_flags(f, kl, base=base + rl["checked"])
            d["add0"] = f[base + lay["add"]:base + lay["add"] + L].copy()
            d["add1"] = f[base + lay["add"] + L:base + lay["add"] + 2 * L].copy()
            steps.append(d)
        return acc[0], acc[1], tuple(sl), steps

    # ---- sealed BSGS matrix-vector product: the diagonals verified on the load that multiplies them (bsgs_sealed.hip) ----
    def seal_diagonals(self, diags: DeviceArray, n1: int, n2: int, stream=None) -> DeviceArray:
        """The seals of the diagonals ``[n2][n1][L][N]``: ``[n2 * n1 * L][2]``, row ``(g * n1 + b) * L + l``."""
        return self.t.seal(diags, limbs=self.L, start=0, n_poly=n1 * n2, stream=stream)

    def bsgs_matvec_sealed_layout(self, n1: int, n2: int):
        """``{"c0", "c1": (offset, (L,)), "baby_keys": (offset, (n1 - 1, dnum, 2, M)), "giant_keys": (offset, (n2 - 1, dnum, 2, M)),
        "diags": (offset, (n2, n1, L)), "checked": offset, "total": n}`` of ``bsgs_matvec_sealed``'s flag buffer; the checked block
        is laid out as ``bsgs_matvec_checked_layout(n1, n2)``."""
        out = (C.c_int * 8)()
        check(lib.fhe_bsgs_matvec_sealed_layout(self._h, n1, n2, out))
        L, M, d = self.L, self.L + self.K, self.dnum
        shapes = ((L,), (L,), (n1 - 1, d, 2, M), (n2 - 1, d, 2, M), (n2, n1, L))
        lay = {name: (int(out[i]), shapes[i]) for i, name in enumerate(("c0", "c1", "baby_keys", "giant_keys", "diags"))}
        lay["checked"], lay["total"] = int(out[5]), int(out[6])
        return lay

    def _bsgs_checked_flags(self, f, n1, n2, base=0):
        """The flag dictionary of ``bsgs_matvec_checked`` from its block, which starts at ``f[base]``."""
        lay = self.bsgs_matvec_checked_layout(n1, n2)
        baby = self._hoisted_flags(f, n1 - 1, base + lay["baby"]) if n1 > 1 else None
        giant = []
        for g in range(n2):
            b0 = base + lay["giant0"] + g * lay["giant_words"]
            blk = self._split_flags(f, lay["giant"], self.BSGS_GIANT_STAGES[:3], b0)
            blk["keyswitch"] = self._split_flags(f, self.checked_layout(), self.CHECKED_STAGES, b0 + lay["giant"]["keyswitch"][0])
            giant.append(blk)
        return {"baby": baby, "giant": giant}

    def bsgs_matvec_sealed(self, c0: DeviceArray, c1: DeviceArray, diags: DeviceArray, n1: int, n2: int, baby_elts, baby_keys_prepared,
                           giant_elts, giant_keys, abft: "Abft", seals=None, baby_key_seals=None, giant_key_seals=None,
                           diag_seal: Optional[DeviceArray] = None, stream=None):
        """``bsgs_matvec_checked`` with the operands protected at rest: ``(o0, o1, (seal0, seal1), flags)``, the words
        ``bsgs_matvec``'s bit for bit.  ``seals`` = the seals of (c0, c1), ``baby_key_seals`` = ``seal_key`` of each PREPARED baby key,
        ``giant_key_seals`` = ``seal_key`` of each giant key, ``diag_seal`` = ``seal_diagonals``; any of them, or an entry, may be
        None: not verified.  c0, c1 and the keys are verified by sweeps of their own; every diagonal word is digested from the
        register that multiplies it, so no diagonal word is read twice and the verified load is the consuming load (n1 > 16: a
        verifying sweep per giant step instead).  ``flags = {"c0", "c1": [L], "baby_keys": [n1 - 1][dnum][2][M], "giant_keys":
        [n2 - 1][dnum][2][M], "diags": [n2][n1][L], "checked": <bsgs_matvec_checked's dict>}``, input words with the bits of
        ``seal_verify``.  A raised input flag does not stop the call."""
        lay = self.bsgs_matvec_sealed_layout(n1, n2)
        be = (C.c_uint32 * max(1, n1 - 1))(*[int(g) for g in baby_elts])
        ge = (C.c_uint32 * max(1, n2 - 1))(*[int(g) for g in giant_elts])
        bk = (vp * max(1, n1 - 1))(*[k.ptr for k in baby_keys_prepared])
        gk = (vp * max(1, n2 - 1))(*[k.ptr for k in giant_keys])

        def ptrs(xs, n):
            return (vp * max(1, n))(*[x.ptr if x is not None else None for x in xs]) if xs is not None else None
        bs, gs = ptrs(baby_key_seals, n1 - 1), ptrs(giant_key_seals, n2 - 1)
        o0, o1, so, f = self._sealed(lay, ("c0", "c1"), self.L, seals, lambda o0, o1, sin, sout, fl: lib.fhe_bsgs_matvec_sealed(
            self.eng._h, self._h, o0.ptr, o1.ptr, c0.ptr, c1.ptr, diags.ptr, n1, n2, be, bk, ge, gk, abft._h, sin, bs, gs,
            diag_seal.ptr if diag_seal is not None else None, sout, fl.ptr, stream), stream)
        flags = self._split_flags(f, lay, ("c0", "c1", "baby_keys", "giant_keys", "diags"))
        flags["checked"] = self._bsgs_checked_flags(f, n1, n2, lay["checked"])
        return o0, o1, so, flags

    # ---- the same composites repairing their operands and key in place (seal_repair.hip) ----
    def seal_key_locator(self, key: DeviceArray, stream=None) -> DeviceArray:
        """The locator sums of a relinearisation or Galois key: ``[dnum * 2 * (L + K)]``, beside ``seal_key``."""
        return self.t.seal_locator(key, limbs=self.L + self.K, start=0, n_poly=2 * self.dnum, stream=stream)

    def _repair_layout(self, out, lay, n):
        lay["report"], lay["flags_total"], lay["total"] = int(out[n]), lay["total"], int(out[n + 1])
        return lay

    def hmult_sealed_repair_layout(self, rescale: bool = True):
        """``hmult_sealed_layout`` plus ``"report"``: the offset, in flag words, of the report block ``[rows][4]`` uint64 over the
        input and key rows in the order of their flag words; ``"flags_total"`` is the sealed layout's total, ``"total"`` includes
        the report block."""
        out = (C.c_int * 10)()
        check(lib.fhe_hmult_sealed_repair_layout(self._h, 1 if rescale else 0, out))
        return self._repair_layout(out, self._sealed_layout(out, ("a0", "a1", "b0", "b1"), 5, 6), 7)

    def rotate_sealed_repair_layout(self):
        """``rotate_sealed_layout`` plus the report block, as ``hmult_sealed_repair_layout``."""
        out = (C.c_int * 8)()
        check(lib.fhe_rotate_sealed_repair_layout(self._h, out))
        return self._repair_layout(out, self._sealed_layout(out, ("c0", "c1"), 3, 4), 5)

    def _sealed_repair(self, lay, names, limbs, seals, locators, call, stream):
        """Run ``call(o0, o1, seal_in, loc_in, seal_out, loc_out, flags)``; returns (o0, o1, seals, locators, flat flags, reports)."""
        o0, o1 = self._out(limbs), self._out(limbs)
        so, lo = [self.eng.alloc(2 * limbs) for _ in range(2)], [self.eng.alloc(limbs) for _ in range(2)]
        for x in so:
            x.shape = (limbs, 2)
        ptrs = lambda xs: (vp * len(names))(*[x.ptr if x is not None else None for x in (tuple(xs) if xs is not None else (None,) * len(names))])
        sout, lout = (vp * 2)(so[0].ptr, so[1].ptr), (vp * 2)(lo[0].ptr, lo[1].ptr)
        flags = _flag_buffer(self.eng, lay["total"])
        check(call(o0, o1, ptrs(seals), ptrs(locators), sout, lout, flags))
        raw = _read_flags(flags, lay["total"], stream).copy()
        rows = lay["checked"]
        report = raw[lay["report"]:lay["report"] + 8 * rows].view(np.uint64).reshape(rows, 4)
        reports = {name: report[lay[name][0]:lay[name][0] + int(np.prod(lay[name][1]))].reshape(lay[name][1] + (4,)).copy() for name in names + ("key",)}
        return o0, o1, tuple(so), tuple(lo), raw, reports

    def hmult_sealed_repair(self, a0: DeviceArray, a1: DeviceArray, b0: DeviceArray, b1: DeviceArray, relin_key: DeviceArray, abft: "Abft",
                            seals=None, locators=None, key_seal: Optional[DeviceArray] = None, key_locator: Optional[DeviceArray] = None,
                            rescale: bool = True, stream=None):
        """``hmult_sealed`` with every given (seal, locator) pair repaired in place instead of only verified -- the operands and the
        key may be WRITTEN: ``(out0, out1, (seal0, seal1), (locator0, locator1), flags, reports)``.  ``locators`` go with ``seals``
        entry by entry (``NttTables.seal_locator``), ``key_locator`` with ``key_seal`` (``seal_key_locator``).  ``flags`` as
        ``hmult_sealed``: a repaired row's flag is clear again, an uncorrectable or suspect row's stays raised and does not stop the
        call.  ``reports = {"a0", ..., "key": [...][4]}`` = {outcome, index, word before, word after} per row."""
        names = ("a0", "a1", "b0", "b1")
        lay = self.hmult_sealed_repair_layout(rescale)
        o0, o1, so, lo, f, rep = self._sealed_repair(lay, names, self.L - 1 if rescale else self.L, seals, locators,
                                                     lambda o0, o1, sin, lin, sout, lout, fl: lib.fhe_hmult_sealed_repair(
            self.eng._h, self._h, o0.ptr, o1.ptr, a0.ptr, a1.ptr, b0.ptr, b1.ptr, relin_key.ptr, 1 if rescale else 0, abft._h, sin, lin,
            key_seal.ptr if key_seal is not None else None, key_locator.ptr if key_locator is not None else None, sout, lout, fl.ptr, stream), stream)
        flags = self._split_flags(f, lay, names + ("key",))
        flags["checked"] = self._hmult_flags(bool(self.plain_modulus), f, rescale, lay["checked"])
        return o0, o1, so, lo, flags, rep

    def rotate_sealed_repair(self, c0: DeviceArray, c1: DeviceArray, galois_elt: int, galois_key: DeviceArray, abft: "Abft", seals=None, locators=None,
                             key_seal: Optional[DeviceArray] = None, key_locator: Optional[DeviceArray] = None, stream=None):
        """``rotate_sealed`` with every given (seal, locator) pair repaired in place: ``(out0, out1, seals, locators, flags,
        reports)`` as ``hmult_sealed_repair``."""
        names = ("c0", "c1")
        lay = self.rotate_sealed_repair_layout()
        o0, o1, so, lo, f, rep = self._sealed_repair(lay, names, self.L, seals, locators,
                                                     lambda o0, o1, sin, lin, sout, lout, fl: lib.fhe_rotate_sealed_repair(
            self.eng._h, self._h, o0.ptr, o1.ptr, c0.ptr, c1.ptr, galois_elt, galois_key.ptr, abft._h, sin, lin,
            key_seal.ptr if key_seal is not None else None, key_locator.ptr if key_locator is not None else None, sout, lout, fl.ptr, stream), stream)
        flags = self._split_flags(f, lay, names + ("key",))
        kl = self._ks_layout(bool(self.plain_modulus))
        flags["checked"] = self._split_flags(f, kl, base=lay["checked"])
        return o0, o1, so, lo, flags, rep

    def __del__(self):
        try:
            if self._h and self.eng._h:
                lib.fhe_keyswitch_destroy(self._h)
        except Exception:
            pass


# ---------------------------------------------------------------------------
# ABFT detector
# ---------------------------------------------------------------------------
class Abft:
    """Weighted-checksum ECC around the forward NTT, the inverse NTT and the negacyclic product
    (rfhe_framewk/src/negaclic_ntt.py:130-149)."""

    def __init__(self, eng: Engine, t: NttTables):
        self.eng, self.t = eng, t
        h = vp()
        check(lib.fhe_abft_create(eng._h, t._h, C.byref(h)))
        self._h = h

    def checksum(self, d: DeviceArray, side: int, n_poly: int = 1, limbs: Optional[int] = None, start: int = 0) -> np.ndarray:
        limbs = len(self.t) - start if limbs is None else limbs
        out = self.eng.alloc(n_poly * limbs)
        check(lib.fhe_abft_checksum(self.eng._h, self._h, side, d.ptr, out.ptr, n_poly, limbs, start, None))
        return out.download()

    def forward_checked(self, d: DeviceArray, n_poly: int = 1, limbs: Optional[int] = None, start: int = 0) -> np.ndarray:
        """In-place forward NTT; returns the per-limb-polynomial fault flags."""
        limbs = len(self.t) - start if limbs is None else limbs
        return _checked_flags(self.eng, n_poly * limbs, lambda fl: lib.fhe_ntt_forward_checked(self.eng._h, d.ptr, self.t._h, self._h, n_poly, limbs, start, fl.ptr,
                                                                                               None))

    def forward_checked_phases(self, d: DeviceArray, n_poly: int = 1, limbs: Optional[int] = None, start: int = 0) -> np.ndarray:
        """In-place forward NTT with the per-phase detector; returns flags[unit, 3] = (column pass, hand-off, row pass)."""
        limbs = len(self.t) - start if limbs is None else limbs
        n = n_poly * limbs * 3
        return _checked_flags(self.eng, n, lambda fl: lib.fhe_ntt_forward_checked_phases(self.eng._h, d.ptr, self.t._h, self._h, n_poly, limbs, start, fl.ptr,
                                                                                         None)).reshape(n_poly * limbs, 3)

    def inverse_checked(self, d: DeviceArray, n_poly: int = 1, limbs: Optional[int] = None, start: int = 0) -> np.ndarray:
        """In-place inverse NTT; returns the per-limb-polynomial fault flags.

        The forward detector's weights with the sides swapped: x = F^-1 x_hat gives sum_j w_hat_j x_hat_j = sum_i w_i x_i, the
        input side weighed with w_hat on the words the first launch loads, the output side with w on the words the last one
        stores -- the check after the closing transform of rfhe_framewk/src/four_step_ntt_protected.py:219-282."""
        limbs = len(self.t) - start if limbs is None else limbs
        return _checked_flags(self.eng, n_poly * limbs, lambda fl: lib.fhe_ntt_inverse_checked(self.eng._h, d.ptr, self.t._h, self._h, n_poly, limbs, start, fl.ptr,
                                                                                               None))

    def polymul_checked(self, c: DeviceArray, a: DeviceArray, b: DeviceArray, n_poly: int = 1, limbs: Optional[int] = None,
                        start: int = 0) -> np.ndarray:
        """c = a * b mod (x^N + 1, q) as ``NttTables.polymul`` (a and b are scratch, c may alias either); returns
        flags[unit, 3] = (forward transform of a, forward transform of b, product + inverse).

        The three checks of the protected chain transform -> element-wise product -> transform
        (rfhe_framewk/src/four_step_ntt_protected.py:219-282): sum w a == sum w_hat a_hat, sum w b == sum w_hat b_hat, and,
        since c_hat_j = a_hat_j b_hat_j, sum_i w_i c_i == sum_j w_hat_j a_hat_j b_hat_j -- the last sum formed next to the
        product, not from its result."""
        limbs = len(self.t) - start if limbs is None else limbs
        n = n_poly * limbs * 3
        return _checked_flags(self.eng, n, lambda fl: lib.fhe_polymul_checked(self.eng._h, c.ptr, a.ptr, b.ptr, self.t._h, self._h, n_poly, limbs, start, fl.ptr,
                                                                              None)).reshape(n_poly * limbs, 3)

    def polymul_sealed(self, c: DeviceArray, a: DeviceArray, b: DeviceArray, seal_a: Optional[DeviceArray], seal_b: Optional[DeviceArray],
                       seal_out: bool = True, n_poly: int = 1, limbs: Optional[int] = None, start: int = 0, stream=None):
        """``polymul_checked`` with the factors' seals verified on the loads that transform them and the seal of ``c`` written from
        the words the last launch stores: ``(seal_c, flags)``.  ``flags`` is a dict of uint32 arrays: ``a[rows]`` and ``b[rows]``
        the factors' verdicts with ``seal_verify``'s bits (a seal that is None is not compared, the window still is), ``checked[rows,
        3]`` ``polymul_checked``'s own flags.  ``seal_c`` is ``[rows][2]``, ``seal``'s of ``c`` word for word on a row with no raised
        flag and ``{~0, ~0}`` otherwise; ``seal_out`` False: no output digest, ``seal_c`` is None.  ``a`` and ``b`` are scratch: their
        seals no longer describe them after the call.  ``c`` may alias either factor; ``b is a`` squares (``seal_b`` None or
        ``seal_a``; ``flags['b']`` repeats ``flags['a']``).  The words are ``polymul``'s, bit for bit; a raised flag does not stop
        the call.  Whole-batch launches only."""
        limbs = len(self.t) - start if limbs is None else limbs
        rows = n_poly * limbs
        seal_c = None
        if seal_out:
            seal_c = self.eng.alloc(rows * 2)
            seal_c.shape = (rows, 2)
        f = _checked_flags(self.eng, 5 * rows, lambda fl: lib.fhe_polymul_sealed(
            self.eng._h, c.ptr, a.ptr, b.ptr, self.t._h, self._h, n_poly, limbs, start, seal_a.ptr if seal_a is not None else None,
            seal_b.ptr if seal_b is not None else None, seal_c.ptr if seal_c is not None else None, fl.ptr, stream), stream)
        return seal_c, {"a": f[:rows], "b": f[rows:2 * rows], "checked": f[2 * rows:].reshape(rows, 3)}

    def __del__(self):
        try:
            if self._h and self.eng._h:
                lib.fhe_abft_destroy(self._h)
        except Exception:
            pass
