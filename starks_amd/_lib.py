"""ctypes binding of libstarkhip.so (C ABI: include/starkhip.h).

There is NO CPU fallback: if the shared library is missing, or no MI355X is visible, every entry point
raises.  Build with `python -c "import __graft_entry__ as g; g.build()"` (or `make -C starks_amd/csrc`).
"""
import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("STARKHIP_LIB") or os.path.join(_HERE, "libstarkhip.so")

MIMC_P = 2**256 - 2**32 * 351 + 1  # starks/utils.py:22

_lib = None
_ctx = None
_ctx2 = None
_lock = threading.Lock()


class StarkHipError(RuntimeError):
    def __init__(self, status, where, detail=""):
        self.status = status
        msg = "%s failed: %s (%d)" % (where, _strerror(status), status)
        if detail:
            msg += " -- " + detail
        super().__init__(msg)


def _strerror(status):
    try:
        return lib().sh_strerror(status).decode()
    except Exception:  # pragma: no cover
        return "status %d" % status


def lib():
    """Load the shared library (no device needed for this step)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "starks_amd: %s is missing -- the HIP extension has not been built. Run "
            "`python -c \"import __graft_entry__ as g; g.build()\"` or `make -C starks_amd/csrc`. "
            "There is no CPU fallback." % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    c_p, u8p, u64, u32, i32 = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    pp = ctypes.POINTER(c_p)
    sig = {
        "sh_strerror": (ctypes.c_char_p, [i32]),
        "sh_version": (ctypes.c_char_p, []),
        "sh_ctx_create": (i32, [i32, pp]),
        "sh_ctx_destroy": (None, [c_p]),
        "sh_last_error": (ctypes.c_char_p, [c_p]),
        "sh_device_count": (i32, []),
        "sh_sync": (i32, [c_p]),
        "sh_timer_start": (i32, [c_p]),
        "sh_timer_stop": (i32, [c_p, ctypes.POINTER(ctypes.c_float)]),
        "sh_ntt": (i32, [c_p, c_p, u64, c_p, u64, u8p, i32]),
        "sh_ntt_batch": (i32, [c_p, c_p, u64, c_p, u64, u32, u8p, i32]),
        "sh_mul_polys": (i32, [c_p, u8p, u64, u8p, u64, c_p, u64, u8p]),
        "sh_power_cycle": (i32, [c_p, u8p, u64, c_p]),
        "sh_lde": (i32, [c_p, u8p, c_p, u64, u32, u32, u8p]),
        "sh_merkelize": (i32, [c_p, u8p, u64, c_p]),
        "sh_merkelize_packed": (i32, [c_p, u8p, u64, u32, c_p, c_p]),
        "sh_fri_fold": (i32, [c_p, u8p, u64, u8p, u8p, c_p]),
        "sh_fri_proof_len": (u64, [u64, u64, u32]),
        "sh_fri_prove": (i32, [c_p, u8p, u64, u64, u8p, u64, u32, u32, u32, c_p, u64]),
        "sh_dev_alloc": (i32, [c_p, u64, pp]),
        "sh_dev_free": (i32, [c_p, c_p]),
        "sh_dev_from_wire": (i32, [c_p, u8p, c_p, u64]),
        "sh_dev_to_wire": (i32, [c_p, c_p, c_p, u64]),
        "sh_dev_download": (i32, [c_p, c_p, c_p, u64]),
        "sh_dev_upload": (i32, [c_p, u8p, c_p, u64]),
        "sh_dev_copy": (i32, [c_p, c_p, c_p, u64]),
        "sh_fri_verify": (i32, [u8p, u64, u8p, u64, u8p, u64, u32, u32]),
        "sh_stark_verify": (i32, [u8p, u64, u8p, u8p, u64, u32, u32, u8p, u8p, ctypes.POINTER(u32), u32]),
        "sh_dev_download_async": (i32, [c_p, c_p, c_p, u64]),
        "sh_io_sync": (i32, [c_p]),
        "sh_host_alloc": (i32, [c_p, u64, pp]),
        "sh_host_free": (i32, [c_p, c_p]),
        "sh_ntt_passes": (u32, [u64, u32]),
        "sh_dev_download_2d": (i32, [c_p, c_p, u64, c_p, u64, u64]),
        "sh_dev_fill_seeded": (i32, [c_p, c_p, u64, u64]),
        "sh_dev_ntt": (i32, [c_p, c_p, c_p, u64, u32, u8p, i32]),
        "sh_dev_lde": (i32, [c_p, c_p, c_p, u64, u32, u32, u8p]),
        "sh_dev_merkelize": (i32, [c_p, c_p, u64, u32, c_p]),
        "sh_dev_fri_fold": (i32, [c_p, c_p, c_p, u64, u32, u8p, c_p]),
        "sh_dev_fri_prove": (i32, [c_p, c_p, u64, u8p, u64, u32, u32, u32, c_p]),
        "sh_dev_fri_prove_coeffs": (i32, [c_p, c_p, u64, u64, u8p, u64, u32, u32, u32, c_p]),
        "sh_stark_proof_len": (u64, [u64, u32, u32, u32, u32]),
        "sh_stark_prove": (i32, [c_p, u8p, u8p, u64, u32, u32, u8p, u8p, c_p, u32, u32, c_p, u64]),
        "sh_dev_stark_prove": (i32, [c_p, c_p, c_p, u64, u32, u32, u8p, u8p, c_p, u32, u32, c_p]),
        "sh_stark_status": (i32, [c_p]),
        "sh_stark_status_batch": (i32, [c_p, c_p, u32]),
        "sh_ctx_trim": (i32, [c_p]),
        "sh_ctx_set_plan_budget": (i32, [c_p, u64]),
        "sh_ctx_stats": (i32, [c_p, ctypes.POINTER(u64)]),
        "sh_dev_fill_mimc_units": (i32, [c_p, c_p, c_p, u64, u32, u32, u32]),
        "sh_dev_stark_verify": (i32, [c_p, c_p, c_p, c_p, u64, u64, u32, u32, u8p, u8p, ctypes.POINTER(u32), u32, u32, c_p]),
        "sh_dev_fri_verify": (i32, [c_p, c_p, c_p, u64, u8p, u64, u32, u32, u32, c_p]),
        "sh_stark_verify_batch": (i32, [c_p, u8p, u64, u8p, u8p, u64, u32, u32, u8p, u8p, ctypes.POINTER(u32), u32, u32, c_p]),
        "sh_fri_verify_batch": (i32, [c_p, u8p, u64, u8p, u64, u8p, u64, u32, u32, u32, c_p]),
        "sh_dev_stark_witness": (i32, [c_p, c_p, u64, u32, u8p, u8p, c_p, u32, c_p]),
        "sh_stark_witness": (i32, [c_p, u8p, u64, u32, u8p, u8p, c_p, u32, c_p, u64]),
        "sh_dev_multi_inv": (i32, [c_p, c_p, c_p, u64]),
        "sh_multi_inv": (i32, [c_p, u8p, u64, c_p]),
        "sh_dev_multi_interp_4": (i32, [c_p, c_p, c_p, u64, c_p]),
        "sh_multi_interp_4": (i32, [c_p, u8p, u8p, u64, c_p]),
        "sh_dev_poly_mul": (i32, [c_p, c_p, u64, c_p, u64, c_p]),
        "sh_poly_mul": (i32, [c_p, u8p, u64, u8p, u64, c_p]),
        "sh_dev_poly_divmod": (i32, [c_p, c_p, u64, c_p, u64, c_p, c_p]),
        "sh_poly_divmod": (i32, [c_p, u8p, u64, u8p, u64, c_p, c_p]),
        "sh_dev_zpoly": (i32, [c_p, c_p, u64, c_p]),
        "sh_zpoly": (i32, [c_p, u8p, u64, c_p]),
        "sh_dev_lagrange_interp": (i32, [c_p, c_p, c_p, u64, c_p]),
        "sh_lagrange_interp": (i32, [c_p, u8p, u8p, u64, c_p]),
        "sh_dev_poly_eval": (i32, [c_p, c_p, u64, u32, c_p, u64, c_p]),
        "sh_poly_eval": (i32, [c_p, u8p, u64, u32, u8p, u64, c_p]),
        "sh_mod_ntt": (i32, [c_p, u8p, u8p, u64, c_p, u64, u32, u8p, i32]),
        "sh_dev_mod_ntt": (i32, [c_p, u8p, c_p, c_p, u64, u32, u8p, i32]),
        "sh_mod_mul_polys": (i32, [c_p, u8p, u8p, u64, u8p, u64, c_p, u64, u8p]),
        "sh_dev_mod64_ntt": (i32, [c_p, u64, c_p, u64, c_p, u64, u32, u64, i32]),
        "sh_mod64_ntt": (i32, [c_p, u64, c_p, u64, c_p, u64, u32, u64, i32]),
        "sh_mod64_mul_polys": (i32, [c_p, u64, c_p, u64, c_p, u64, c_p, u64, u64]),
        "sh_dev_mod64_from_limbs": (i32, [c_p, u64, c_p, c_p, u64]),
        "sh_dev_mod64_to_limbs": (i32, [c_p, c_p, c_p, u64]),
        "sh_mod_fri_prove": (i32, [c_p, u8p, u8p, u64, u64, u8p, u64, u32, u32, u32, c_p, u64]),
        "sh_dev_mod_fri_prove": (i32, [c_p, u8p, c_p, u64, u64, u8p, u64, u32, u32, u32, c_p]),
        "sh_mod_fri_fold": (i32, [c_p, u8p, u8p, u64, u8p, u8p, c_p]),
        "sh_dev_merkelize_plain": (i32, [c_p, c_p, u64, u32, c_p]),
        "sh_mod64_fri_prove": (i32, [c_p, u64, c_p, u64, u64, u64, u64, u32, u32, u32, c_p, u64]),
        "sh_dev_mod64_fri_prove": (i32, [c_p, u64, c_p, u64, u64, u64, u64, u32, u32, u32, c_p]),
        "sh_mod64_fri_fold": (i32, [c_p, u64, c_p, u64, u64, u8p, c_p]),
        "sh_dev_mod64_merkelize": (i32, [c_p, c_p, u64, u32, c_p]),
        "sh_mod_fri_verify": (i32, [u8p, u8p, u64, u8p, u64, u8p, u64, u32, u32]),
        "sh_dev_mod_fri_verify": (i32, [c_p, u8p, c_p, c_p, u64, u8p, u64, u32, u32, u32, c_p]),
        "sh_mod_fri_verify_batch": (i32, [c_p, u8p, u8p, u64, u8p, u64, u8p, u64, u32, u32, u32, c_p]),
        "sh_mod_stark_prove": (i32, [c_p, u8p, u8p, u8p, u64, u32, u32, u8p, u8p, c_p, u32, u32, c_p, u64]),
        "sh_dev_mod_stark_prove": (i32, [c_p, u8p, c_p, c_p, u64, u32, u32, u8p, u8p, c_p, u32, u32, c_p]),
        "sh_mod_stark_verify": (i32, [u8p, u8p, u64, u8p, u8p, u64, u32, u32, u8p, u8p, ctypes.POINTER(u32), u32]),
        "sh_dev_mod_stark_verify": (i32, [c_p, u8p, c_p, c_p, c_p, u64, u64, u32, u32, u8p, u8p, ctypes.POINTER(u32), u32, u32, c_p]),
        "sh_mod_stark_verify_batch": (i32, [c_p, u8p, u8p, u64, u8p, u8p, u64, u32, u32, u8p, u8p, ctypes.POINTER(u32), u32, u32, c_p]),
        "sh_dev_mod_stark_witness": (i32, [c_p, u8p, c_p, u64, u32, u8p, u8p, c_p, u32, c_p]),
        "sh_mod_stark_witness": (i32, [c_p, u8p, u8p, u64, u32, u8p, u8p, c_p, u32, c_p, u64]),
        "sh_mod64_stark_prove": (i32, [c_p, u64, c_p, c_p, u64, u32, u32, u8p, u8p, c_p, u32, u32, c_p, u64]),
        "sh_dev_mod64_stark_prove": (i32, [c_p, u64, c_p, c_p, u64, u32, u32, u8p, u8p, c_p, u32, u32, c_p]),
        "sh_dev_mod64_stark_witness": (i32, [c_p, u64, c_p, u64, u32, u8p, u8p, c_p, u32, c_p]),
        "sh_mod64_stark_witness": (i32, [c_p, u64, c_p, u64, u32, u8p, u8p, c_p, u32, c_p, u64]),
        "sh_mod_poly_max_transform": (u64, [i32, u64, u64]),
        "sh_dev_mod_multi_inv": (i32, [c_p, u8p, c_p, c_p, u64]),
        "sh_mod_multi_inv": (i32, [c_p, u8p, u8p, u64, c_p]),
        "sh_dev_mod_multi_interp_4": (i32, [c_p, u8p, c_p, c_p, u64, c_p]),
        "sh_mod_multi_interp_4": (i32, [c_p, u8p, u8p, u8p, u64, c_p]),
        "sh_dev_mod_poly_mul": (i32, [c_p, u8p, u8p, u32, c_p, u64, c_p, u64, c_p]),
        "sh_mod_poly_mul": (i32, [c_p, u8p, u8p, u32, u8p, u64, u8p, u64, c_p]),
        "sh_dev_mod_poly_divmod": (i32, [c_p, u8p, u8p, u32, c_p, u64, c_p, u64, c_p, c_p]),
        "sh_mod_poly_divmod": (i32, [c_p, u8p, u8p, u32, u8p, u64, u8p, u64, c_p, c_p]),
        "sh_dev_mod_zpoly": (i32, [c_p, u8p, u8p, u32, c_p, u64, c_p]),
        "sh_mod_zpoly": (i32, [c_p, u8p, u8p, u32, u8p, u64, c_p]),
        "sh_dev_mod_lagrange_interp": (i32, [c_p, u8p, u8p, u32, c_p, c_p, u64, c_p]),
        "sh_mod_lagrange_interp": (i32, [c_p, u8p, u8p, u32, u8p, u8p, u64, c_p]),
        "sh_dev_mod_poly_eval": (i32, [c_p, u8p, u8p, u32, c_p, u64, u32, c_p, u64, c_p]),
        "sh_mod_poly_eval": (i32, [c_p, u8p, u8p, u32, u8p, u64, u32, u8p, u64, c_p]),
        "sh_dev_mod64_multi_inv": (i32, [c_p, u64, c_p, c_p, u64]),
        "sh_mod64_multi_inv": (i32, [c_p, u64, c_p, u64, c_p]),
        "sh_dev_mod64_multi_interp_4": (i32, [c_p, u64, c_p, c_p, u64, c_p]),
        "sh_mod64_multi_interp_4": (i32, [c_p, u64, c_p, c_p, u64, c_p]),
        "sh_dev_mod64_poly_mul": (i32, [c_p, u64, u64, u32, c_p, u64, c_p, u64, c_p]),
        "sh_mod64_poly_mul": (i32, [c_p, u64, u64, u32, c_p, u64, c_p, u64, c_p]),
        "sh_dev_mod64_poly_divmod": (i32, [c_p, u64, u64, u32, c_p, u64, c_p, u64, c_p, c_p]),
        "sh_mod64_poly_divmod": (i32, [c_p, u64, u64, u32, c_p, u64, c_p, u64, c_p, c_p]),
        "sh_dev_mod64_zpoly": (i32, [c_p, u64, u64, u32, c_p, u64, c_p]),
        "sh_mod64_zpoly": (i32, [c_p, u64, u64, u32, c_p, u64, c_p]),
        "sh_dev_mod64_lagrange_interp": (i32, [c_p, u64, u64, u32, c_p, c_p, u64, c_p]),
        "sh_mod64_lagrange_interp": (i32, [c_p, u64, u64, u32, c_p, c_p, u64, c_p]),
        "sh_dev_mod64_poly_eval": (i32, [c_p, u64, u64, u32, c_p, u64, u32, c_p, u64, c_p]),
        "sh_mod64_poly_eval": (i32, [c_p, u64, u64, u32, c_p, u64, u32, c_p, u64, c_p]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)  # AttributeError here = the library does not export what the header declares
        fn.restype = res
        fn.argtypes = args
    L._sig = sig
    _lib = L
    return L


EXPORTED = None  # filled lazily by exported_symbols()


def exported_symbols():
    """Names bound above == every function include/starkhip.h declares (checked by tests)."""
    return sorted(lib()._sig.keys())


def default_device():
    for var in ("STARKHIP_DEVICE", "LOCAL_RANK"):
        if os.environ.get(var, "") != "":
            return int(os.environ[var])
    return 0


def ctx():
    """The process-wide context (one process per GPU; device = $STARKHIP_DEVICE or $LOCAL_RANK or 0)."""
    global _ctx
    with _lock:
        if _ctx is None:
            L = lib()
            h = ctypes.c_void_p()
            rc = L.sh_ctx_create(default_device(), ctypes.byref(h))
            if rc != 0:
                raise StarkHipError(rc, "sh_ctx_create", "an MI355X (gfx950) GPU is required; there is no CPU fallback")
            _ctx = h
        return _ctx


def second_ctx():
    """A second context on the same GPU (its own stream, workspaces and plan cache; include/starkhip.h: contexts are
    independent), created on first use and kept for the life of the process: the many-proof driver pipelines two batches."""
    global _ctx2
    ctx()
    with _lock:
        if _ctx2 is None:
            h = ctypes.c_void_p()
            rc = lib().sh_ctx_create(default_device(), ctypes.byref(h))
            if rc != 0:
                raise StarkHipError(rc, "sh_ctx_create", "second context")
            _ctx2 = h
        return _ctx2


def close():
    global _ctx, _ctx2
    with _lock:
        if _ctx2 is not None:
            lib().sh_ctx_destroy(_ctx2)
            _ctx2 = None
        if _ctx is not None:
            lib().sh_ctx_destroy(_ctx)
            _ctx = None


def check(rc, where):
    if rc != 0:
        detail = ""
        if _ctx is not None:
            detail = lib().sh_last_error(_ctx).decode()
        raise StarkHipError(rc, where, detail)


class PinnedBuffer(object):
    """`nbytes` of page-locked host memory (sh_host_alloc): a buffer the host-buffer entry points copy to and from the
    GPU without the staging memcpy.  Usable wherever bytes-like data is passed (`buf.view` is a ctypes char array)."""

    def __init__(self, nbytes):
        self.ptr = ctypes.c_void_p()
        check(lib().sh_host_alloc(ctx(), nbytes, ctypes.byref(self.ptr)), "sh_host_alloc")
        self.nbytes = nbytes
        self.view = (ctypes.c_char * nbytes).from_address(self.ptr.value)

    def close(self):
        """Frees the buffer; `view` is dropped with it.  The page-locked allocation belongs to the process, not to the context
        (sh_ctx_destroy frees no caller buffers): after `_lib.close()` it is released through the context-less form
        sh_host_free(NULL, ptr) instead of being leaked."""
        ptr, self.ptr, self.view = self.ptr, None, None
        if ptr:
            rc = lib().sh_host_free(_ctx, ptr)  # _ctx may be None
            if _ctx is not None:
                check(rc, "sh_host_free")
            elif rc != 0:
                raise StarkHipError(rc, "sh_host_free", "")

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def to_wire(values, modulus=MIMC_P):
    """list of ints / field elements -> concatenated 32-byte big-endian strings (modp.py:94-95).

    Values already in [0, 2^256) are sent as they are (an element built from bytes may be unreduced,
    modp.py:33-34; the device reduces); anything else is reduced first, as `field(int)` would.

    One C-level `int.to_bytes` per value and one join (0.3 us per value; the per-value slice assignment this replaces
    took twice that); plain ints in range -- the common case -- take the first branch without any per-value test."""
    wb = getattr(values, "wire_bytes", None)
    if wb is not None:  # a WireList (wireseq.py): the bytes the device wrote, as they are
        return wb()
    if not isinstance(values, (list, tuple)):
        values = list(values)  # an iterator must not be half consumed by the fast path before the general one starts over
    try:
        return b"".join([v.to_bytes(32, "big") for v in values])
    except (AttributeError, OverflowError, TypeError):
        pass  # field elements (no int.to_bytes signature), negative or >= 2^256 values: the general path
    lim = 1 << 256
    ints = [int(v) for v in values]
    return b"".join([(x if 0 <= x < lim else x % modulus).to_bytes(32, "big") for x in ints])


def from_wire(buf):
    """concatenated 32-byte big-endian strings -> list of ints (0.17 us per value)."""
    mv, conv = memoryview(buf), int.from_bytes
    return [conv(mv[i:i + 32], "big") for i in range(0, len(mv), 32)]


def order_of_root(root, modulus=MIMC_P):
    """Multiplicative order of `root` if it is a power of two <= 2^32 (the 2-adic part of p-1), else None.
    The reference gets the same number by walking the powers until they return to 1 (fft.py:319-321)."""
    t = int(root) % modulus
    n = 1
    for _ in range(33):
        if t == 1:
            return n
        t = t * t % modulus
        n *= 2
    return None


# ---- roots of unity and primality for the polynomial entries over a run-time modulus (sh_mod_poly_*) ----------------------------------
MOD_POLY_MUL, MOD_POLY_DIVMOD, MOD_POLY_ZPOLY, MOD_POLY_LAGRANGE, MOD_POLY_EVAL = 0, 1, 2, 3, 4  # sh_mod_poly_max_transform's op
MAX_ROOT_LOG = 26  # the generic transform's largest size
_two_adic = {}
_prime = {}
_MR_BASES = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41)


def is_probable_prime(p):
    """Miller-Rabin on fixed bases, cached per p.  It guards ROUTING (a composite modulus must keep the host path, where the
    reference's algorithms are defined for it), not a correctness claim: the device entries take the caller's word for primality."""
    p = int(p)
    hit = _prime.get(p)
    if hit is not None:
        return hit
    if p < 2:
        res = False
    elif p in _MR_BASES:
        res = True
    elif any(p % b == 0 for b in _MR_BASES):
        res = False
    else:
        d, s = p - 1, 0
        while d % 2 == 0:
            d, s = d // 2, s + 1
        res = True
        for a in _MR_BASES:
            x = pow(a, d, p)
            if x in (1, p - 1):
                continue
            for _ in range(s - 1):
                x = x * x % p
                if x == p - 1:
                    break
            else:
                res = False
                break
    _prime[p] = res
    return res


def two_adic_root(p):
    """(root, k) for an odd prime p: a root of unity of order exactly 2^k, k = min(v2(p - 1), 26), as the sh_mod_poly_* entries take
    it -- g^((p - 1) >> k) for the smallest g >= 2 with g^((p - 1) / 2) = -1 (a quadratic non-residue, so the power has the full
    order).  Cached per p.  Any root of that order gives the same results: they are exact polynomial identities."""
    p = int(p)
    hit = _two_adic.get(p)
    if hit is None:
        if p < 3 or p % 2 == 0:
            raise ValueError("two_adic_root needs an odd prime")
        s = ((p - 1) & -(p - 1)).bit_length() - 1
        g = 2
        while pow(g, (p - 1) // 2, p) != p - 1:
            g += 1
            if g > 1000:
                raise ValueError("no quadratic non-residue below 1000: %d is not prime" % p)
        k = min(s, MAX_ROOT_LOG)
        hit = _two_adic[p] = (pow(g, (p - 1) >> k, p), k)
    return hit


def mod_poly_args(modulus, root=None):
    """(modulus bytes, root bytes, root_log) of a sh_mod_poly_* call; root = None: two_adic_root(modulus), else (root, root_log)"""
    m = int(modulus)
    w, k = two_adic_root(m) if root is None else root
    return m.to_bytes(32, "big"), (int(w) % m).to_bytes(32, "big"), int(k)


def mod64_poly_args(modulus, root=None):
    """(modulus, root, root_log) of a sh_mod64_poly_* call, plain ints; root = None: two_adic_root(modulus), else (root, root_log)"""
    m = int(modulus)
    if not 3 <= m < 1 << 64:
        raise ValueError("the packed-word entries take a modulus in [3, 2^64)")
    w, k = two_adic_root(m) if root is None else root
    return m, int(w) % m, int(k)


def mod_poly_routable(p, op, n_a, n_b=0):
    """The field half of the routing rule of Polynomial and poly_utils over IntegersModP(p), p not the MiMC prime: this process
    already holds a context (read as an attribute: the rule never creates one and never loads the library), p is odd, below 2^256
    and passes the prime test, and the call's largest transform (sh_mod_poly_max_transform) fits the field's 2-adicity."""
    if _ctx is None:
        return False
    p = int(p)
    if p == MIMC_P or p < 3 or p % 2 == 0 or p >> 256 or not is_probable_prime(p):
        return False
    if op is None:  # multi_inv, multi_interp_4: no transform; evaluation: the direct path is always available
        return True
    return lib().sh_mod_poly_max_transform(op, n_a, n_b) <= 1 << two_adic_root(p)[1]
