"""Loader of libcubeslam_hip.so (the C-ABI in include/cubeslam_hip.h and the extension headers include/cubeslam_hip/*.h).  No CPU
fallback: if the library or a HIP device is missing this raises."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CUBESLAM_LIB") or os.path.join(_HERE, "libcubeslam_hip.so")  # CUBESLAM_LIB: a development build of the same library (profiling variants)
_LIB = None

CS_OK = 0
STATUS = {0: "CS_OK", -1: "CS_ERR_NO_DEVICE", -2: "CS_ERR_BAD_ARG", -3: "CS_ERR_HIP", -4: "CS_ERR_CAPACITY", -5: "CS_ERR_NOMEM"}


class CubeSlamError(RuntimeError):
    pass


def build(force=False):
    """Compile every HIP source for gfx950 (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-s", "-C", os.path.join(_HERE, "csrc"), "clean"])
    subprocess.check_call(["make", "-s", "-C", os.path.join(_HERE, "csrc")])


HEADER = os.path.join(os.path.dirname(_HERE), "include", "cubeslam_hip.h")  # the contract: CS_VERSION and every signature are read from it
EXTENSION_DIR = os.path.join(os.path.dirname(_HERE), "include", "cubeslam_hip")  # extension headers: more functions beside an unchanged main header, each with a version of its own


def extension_headers():
    """The extension headers of this tree, by path."""
    return sorted(glob.glob(os.path.join(EXTENSION_DIR, "*.h")))


def extension_version(text):
    """(NAME, value) of the `#define CS_<NAME>_VERSION n` an extension header carries: the library answers cs_<name>_version()."""
    m = re.search(r"#define\s+CS_(\w+)_VERSION\s+(\d+)", text)
    return (m.group(1).lower(), int(m.group(2))) if m else None


def header_version(text=None):
    """CS_VERSION of include/cubeslam_hip.h in this tree."""
    m = re.search(r"#define\s+CS_VERSION\s+(\d+)", open(HEADER).read() if text is None else text)
    return int(m.group(1)) if m else None


_SCALARS = {"int": C.c_int, "long": C.c_long, "float": C.c_float, "double": C.c_double}  # what the header passes by value
_POINTEES = dict(_SCALARS, **{"uint8_t": C.c_uint8, "unsigned char": C.c_ubyte, "uint32_t": C.c_uint32, "int16_t": C.c_int16})


def _ctype(decl, fn):
    """ctypes type of one parameter or return type of the header (`const float *prev_pts`, `long out[6]`, `cs_orb **out`, `void`)."""
    words = re.sub(r"\b(const|volatile)\b|\*|\[\d*\]", " ", decl).split()
    depth = decl.count("*") + decl.count("[")
    base = " ".join(words)
    if len(words) > 1 and base not in _POINTEES:  # the last word is the parameter's name
        base = " ".join(words[:-1])
    if base == "cs_allreduce_fn" and depth == 0:
        return C.c_void_p
    if depth and (base == "void" or re.fullmatch(r"cs_\w+", base)):
        return C.c_void_p
    if base == "char" and depth == 1:
        return C.c_char_p
    t = (_POINTEES if depth else _SCALARS).get(base)
    if t is None:
        raise CubeSlamError("include/cubeslam_hip.h: %s has a type the bindings do not know: '%s'" % (fn, " ".join(decl.split())))
    for _ in range(depth):
        t = C.POINTER(t)
    return t


def signatures(text):
    """{function: (restype, argtypes)} of every `<return type> cs_<name>(<parameters>);` the header text declares; a type outside
    the header's closed set raises CubeSlamError (there is no untyped entry)."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    sigs = {}
    for ret, fn, params in re.findall(r"^([A-Za-z_][\w \t*]*?)\b(cs_\w+)\s*\(([^()]*)\)\s*;", text, flags=re.M):
        params = [] if params.strip() in ("", "void") else params.split(",")
        sigs[fn] = (None if ret.strip() == "void" else _ctype(ret, fn), [_ctype(p, fn) for p in params])
    return sigs


def lib():
    """The library with argtypes and restype of every declared function set from the header: a wrong dtype, a missing pointer or
    a wrong scalar is a ctypes.ArgumentError on the host, before the function is entered."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise CubeSlamError("libcubeslam_hip.so is not built (run python -c 'import __graft_entry__ as g; g.build()')")
        L = C.CDLL(LIB_PATH)
        text = open(HEADER).read()
        extensions = [open(h).read() for h in extension_headers()]
        for header in [text] + extensions:  # one table: the main header's signatures and every extension header's
            for fn, (restype, argtypes) in signatures(header).items():
                if hasattr(L, fn):  # a declared function the library does not export is test_cabi's finding
                    f = getattr(L, fn)
                    f.restype, f.argtypes = restype, argtypes
        want = header_version(text)
        if L.cs_version() != want:  # an ABI-changing header with a stale library (or the reverse) must not get as far as a call
            raise CubeSlamError("libcubeslam_hip.so is version %d, include/cubeslam_hip.h is %s: rebuild" % (L.cs_version(), want))
        for header in extensions:
            name, value = extension_version(header) or (None, None)
            if name and (not hasattr(L, "cs_%s_version" % name) or getattr(L, "cs_%s_version" % name)() != value):
                raise CubeSlamError("libcubeslam_hip.so does not hold version %d of include/cubeslam_hip/%s.h: rebuild" % (value, name))
        _LIB = L
    return _LIB


_PTR = {}


def ptr(a):
    """Pointer to a's data for a cs_* call, typed by a.dtype (ctypes compares it with the header's parameter at the call);
    void * for a structured dtype (the cs_* structs); None stays NULL.  No contiguity demand: strided frames pass their stride."""
    if a is None:
        return None
    t = _PTR.get(a.dtype)
    if t is None:
        t = _PTR[a.dtype] = C.c_void_p if a.dtype.fields else C.POINTER(np.ctypeslib.as_ctypes_type(a.dtype))
    return a.ctypes.data_as(t)


def check(ctx, r, what):
    if r != CS_OK:
        msg = lib().cs_last_error(ctx).decode() if ctx else ""
        raise CubeSlamError("%s failed: %s %s" % (what, STATUS.get(r, r), msg))


class Handle:
    """close() and __del__ of a wrapper that owns one library handle: the attribute named HANDLE holds it and the function named
    DESTROY frees it, behind the context (self.ctx) where the header's destroy takes one."""
    HANDLE = DESTROY = None

    def close(self):
        h = getattr(self, self.HANDLE)
        if h:
            destroy = getattr(lib(), self.DESTROY)
            destroy(*((self.ctx.ptr, h) if len(destroy.argtypes) == 2 else (h,)))
            setattr(self, self.HANDLE, C.c_void_p())

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """cs_ctx wrapper: one HIP device + stream."""

    def __init__(self, device=0, priority=0):
        self._ctx = C.c_void_p()
        r = lib().cs_create_with_priority(int(device), int(priority), C.byref(self._ctx))
        if r != CS_OK:
            raise CubeSlamError("cs_create(device=%d) failed: %s (no HIP device? this package has no CPU path)" % (device, STATUS.get(r, r)))

    @property
    def ptr(self):
        return self._ctx

    def sync(self):
        check(self._ctx, lib().cs_sync(self._ctx), "cs_sync")

    def timing(self, on=True):
        check(self._ctx, lib().cs_timing_enable(self._ctx, int(on)), "cs_timing_enable")

    def timing_reset(self):
        check(self._ctx, lib().cs_timing_reset(self._ctx), "cs_timing_reset")

    def timing_get(self, name):
        ms, n = C.c_double(), C.c_long()
        check(self._ctx, lib().cs_timing_get(self._ctx, name.encode(), C.byref(ms), C.byref(n)), "cs_timing_get")
        return ms.value, n.value

    @staticmethod
    def comm_unique_id():
        """ncclUniqueId (128 bytes): rank 0 creates it, every rank passes the same bytes to comm_init."""
        buf = (C.c_ubyte * 128)()
        r = lib().cs_comm_unique_id(buf)
        if r != CS_OK:
            raise CubeSlamError("cs_comm_unique_id failed: %s" % STATUS.get(r, r))
        return bytes(buf)

    def comm_init(self, rank, world, unique_id):
        """RCCL communicator of this rank on the context's stream (cs_comm_init)."""
        buf = (C.c_ubyte * 128).from_buffer_copy(bytes(unique_id))
        check(self._ctx, lib().cs_comm_init(self._ctx, int(rank), int(world), buf), "cs_comm_init")

    def close(self):
        if self._ctx:
            lib().cs_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
