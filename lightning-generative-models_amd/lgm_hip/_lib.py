"""ctypes binding of liblgm_hip.so.  Signatures are parsed from include/lgm_hip.h so the Python
side can never drift from the C-ABI; loading fails loudly when the library is missing (there
is NO fallback path: the product is the HIP library)."""
from __future__ import annotations

import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
_PKG = os.path.dirname(_HERE)
# LGM_LIB=<path>: another build of the same library (A/B runs of compile-time experiment knobs); default: the in-tree one
LIB_PATH = os.environ.get("LGM_LIB") or os.path.join(_PKG, "csrc", "liblgm_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "lgm_hip.h")


class ConvGeom(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in
                ("B", "H", "W", "Cw", "Ho", "Wo", "Nw", "KH", "KW", "stride", "pad")]


_CTYPES = {
    "int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double,
    "void": None,
}


def _ctype(decl: str):
    decl = decl.replace("const", "").strip()
    if "*" in decl:
        base = decl.replace("*", "").strip()
        if base == "char":
            return ctypes.c_char_p
        return ctypes.c_void_p  # every pointer crosses as a raw address
    return _CTYPES[decl]


def parse_header(path: str = HEADER_PATH):
    """-> {name: (restype, [argtypes])} for every lgm_* prototype in the header."""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"^\s*#[^\n]*", "", text, flags=re.M)      # preprocessor lines
    text = re.sub(r"typedef\s+struct\s*\{.*?\}\s*\w+\s*;", "", text, flags=re.S)
    text = text.replace('extern "C" {', "")
    protos = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(lgm_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        argtypes = []
        if args and args != "void":
            for a in args.split(","):
                a = " ".join(a.split())
                # drop the parameter name (last identifier)
                tdecl = re.sub(r"\b\w+$", "", a).strip() if not a.endswith("*") else a
                argtypes.append(_ctype(tdecl))
        protos[name] = (_ctype(ret), argtypes)
    return protos


def source_fingerprint() -> dict:
    """{file name: sha256 prefix} of every source liblgm_hip.so is built from (csrc/*.hip, csrc/*.h, include/*.h).
    tools/pmc_kernels.py stores it beside the counter summary it writes; bench.py compares it with the tree it runs from
    and refuses a ``roofline.traffic`` figure measured on other kernel code (a committed counter file
    "silently goes stale when a kernel changes after the last PMC pass").  Content, not mtime: snapshots do not keep times."""
    import glob
    import hashlib
    out = {}
    for f in sorted(glob.glob(os.path.join(_PKG, "csrc", "*.hip")) + glob.glob(os.path.join(_PKG, "csrc", "*.h"))
                    + glob.glob(os.path.join(os.path.dirname(_PKG), "include", "*.h"))):
        with open(f, "rb") as fh:
            out[os.path.basename(f)] = hashlib.sha256(fh.read()).hexdigest()[:16]
    return out


def header_abi_version(path: str = HEADER_PATH) -> int:
    m = re.search(r"#define\s+LGM_ABI_VERSION\s+(\d+)", open(path).read())
    return int(m.group(1))


ABI_VERSION = header_abi_version()


# Process-wide knobs that change which kernels the planners pick and how large their workspaces are.  Everything host-side
# that caches a plan per geometry (lgm_hip/ops.py) registers a hook here; the hooks run after EVERY call of one of these
# entry points through lib(), whoever makes it, so a plan cached under one selection can never be used under another
# (VERDICT r5 weak 11 / ADVICE r5: a light-mode GroupNorm-statistics row count reused in 32-tile mode).
_SELECTION_KNOBS = ("lgm_set_cu_margin", "lgm_wino4_set_light")
_SELECTION_HOOKS = []


def on_selection_change(hook):
    if hook not in _SELECTION_HOOKS:
        _SELECTION_HOOKS.append(hook)


class LgmError(RuntimeError):
    """A C-ABI entry point returned non-zero.  The convention of include/lgm_hip.h: rc < 0 = the HOST rejected the
    call (argument / geometry / unsupported shape: nothing was launched, the device is fine), rc > 0 = a hipError_t
    from a launch or the runtime (the device state is suspect)."""


class LgmArgumentError(LgmError):
    """rc < 0: rejected on the host before any launch."""


class LgmDeviceError(LgmError):
    """rc > 0: a hipError_t; callers must not keep using the device (no state_dict(), no further launches)."""


class _Lib:
    def __init__(self):
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: build it with `python __graft_entry__.py build` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        # torch first: liblgm_hip.so must bind to the HIP runtime torch ships (same SONAME).  Loaded on its own it
        # pulls in /opt/rocm's copy, torch then brings a second one, and launches on torch's streams fail with
        # "no ROCm-capable device is detected".
        import torch  # noqa: F401
        self._dll = ctypes.CDLL(LIB_PATH)
        self.protos = parse_header()
        self._dll.lgm_abi_version.restype = ctypes.c_int
        built = self._dll.lgm_abi_version()
        if built != ABI_VERSION:      # a stale .so against a newer header: signatures would be mis-bound silently
            raise ImportError(f"{LIB_PATH} was built for ABI {built}, include/lgm_hip.h declares {ABI_VERSION}: "
                              "rebuild it (python __graft_entry__.py build)")
        self._dll.lgm_last_error.restype = ctypes.c_char_p
        self._dll.lgm_last_kernel.restype = ctypes.c_char_p
        for name, (res, args) in self.protos.items():
            fn = getattr(self._dll, name)  # AttributeError if the .so misses a declared symbol
            fn.restype = res
            fn.argtypes = args
            if res is ctypes.c_int and name not in ("lgm_abi_version", "lgm_kernel_name_count", "lgm_cu_margin",
                                                    "lgm_wgrad_queue_enable"):      # (returns the previous state)
                call = self._checked(fn, name)
                if name in _SELECTION_KNOBS:
                    call = self._with_selection_hooks(call, name)
                setattr(self, name, call)
            else:
                setattr(self, name, fn)

    @staticmethod
    def _with_selection_hooks(call, name):
        def knob(*a):
            call(*a)
            for hook in _SELECTION_HOOKS:
                hook()
        knob.__name__ = name
        return knob

    def _checked(self, fn, name):
        last_error = self._dll.lgm_last_error

        def call(*a):
            rc = fn(*a)
            if rc != 0:
                raise (LgmDeviceError if rc > 0 else LgmArgumentError)(f"{name} failed (rc={rc}): {last_error().decode()}")
        call.__name__ = name
        return call


_lib = None


def lib() -> _Lib:
    global _lib
    if _lib is None:
        _lib = _Lib()
    return _lib
