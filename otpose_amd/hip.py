"""ctypes binding of the C-ABI library ``libotpose_hip.so``, derived from its header include/otpose_hip.h.

The library is built in-tree by ``__graft_entry__.build()`` (``make -C otpose_amd/csrc``).  There is
no fallback: :func:`lib` raises if the shared object is missing, and every operator raises if its
tensors are not on a GPU.

The header is the single source of the binding: :func:`parse_header` reads it once at import and yields
``SIGNATURES`` (name -> (restype, argtypes) of every ``int|size_t otp_*(...);`` prototype), one
``ctypes.Structure`` per ``typedef struct otp_*_desc`` (``ConvDesc``, ``NhwcConvDesc``, ``H16ConvDesc``: the fields
in declaration order) and ``CONSTANTS`` (every ``#define OTP_* <integer>``).  A parameter maps by this rule alone:

    int, float, double, size_t, unsigned long long    c_int, c_float, c_double, c_size_t, c_ulonglong
    a pointer to void at any constness and depth      c_void_p     (device memory, streams, arrays of device pointers)
    int*, double*                                     POINTER(c_int), POINTER(c_double)      (host memory)
    const otp_X_desc*                                 POINTER(the Structure of otp_X_desc)   (host memory)

Parameters are named in the header; anything the rule does not cover is an error that names the prototype.  A constant
is read only when its value is a decimal integer (optionally in parentheses); one written any other way is absent from
``CONSTANTS`` and a lookup of it fails with ``KeyError``.
"""
from __future__ import annotations

import ctypes
import os
import re
import threading
from ctypes import POINTER, c_double, c_float, c_int, c_size_t, c_ulonglong, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OTPOSE_HIP_LIB") or os.path.join(_HERE, "csrc", "libotpose_hip.so")   # env: dev builds
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "otpose_hip.h")
_lib = None
_tls = threading.local()          # device of the tensor the latest stream_of() was asked about (per thread)

_SCALARS = {"int": c_int, "float": c_float, "double": c_double, "size_t": c_size_t, "unsigned long long": c_ulonglong}
_HOST_POINTERS = {"int": POINTER(c_int), "double": POINTER(c_double)}


def _param(decl, proto, structs):
    """ctypes type of one named parameter declaration of prototype ``proto`` (the rule of the module docstring)."""
    words = [t for t in re.findall(r"\w+|\*", decl) if t != "const"]
    depth = words.count("*")
    base = " ".join(w for w in words[:-1] if w != "*")
    if depth == 0 and base in _SCALARS:
        return _SCALARS[base]
    if depth and base == "void":
        return c_void_p
    if depth == 1 and base in _HOST_POINTERS:
        return _HOST_POINTERS[base]
    if depth == 1 and base in structs:
        return POINTER(structs[base])
    raise ValueError(f"{proto}: no ctypes mapping for parameter '{' '.join(decl.split())}'")


def parse_header(text):
    """(signatures, structs, constants) of the text of a C header written like include/otpose_hip.h."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants = {n: int(v) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(OTP_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, re.M)}
    structs = {}
    for name, body in re.findall(r"typedef\s+struct\s+(otp_\w+)\s*\{(.*?)\}\s*\1\s*;", text, re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            ctype, names = decl.split(None, 1)
            if ctype not in ("int", "float"):
                raise ValueError(f"struct {name}: no ctypes mapping for field declaration '{decl}'")
            fields += [(n.strip(), _SCALARS[ctype]) for n in names.split(",")]
        cls = "".join(w.capitalize() for w in name.split("_")[1:])                 # otp_nhwc_conv_desc -> NhwcConvDesc
        structs[name] = type(cls, (ctypes.Structure,), {"_fields_": fields, "__doc__": f"``{name}`` (include/otpose_hip.h)."})
    signatures = {}
    for res, name, params in re.findall(r"\b(int|size_t)\s+(otp_\w+)\s*\(([^()]*)\)\s*;", text):
        params = [] if params.strip() in ("", "void") else params.split(",")
        signatures[name] = (_SCALARS[res], [_param(p, name, structs) for p in params])
    return signatures, structs, constants


def _read_header():
    if not os.path.isfile(HEADER_PATH):
        raise RuntimeError(f"C header {HEADER_PATH} is missing - the ctypes binding of libotpose_hip.so is derived from it "
                           "(a source checkout keeps it next to the package). otpose_amd has no CPU or PyTorch-op fallback.")
    with open(HEADER_PATH) as f:
        return parse_header(f.read())


# name -> (restype, argtypes); kept in one table so tests can check every symbol is exported
SIGNATURES, _STRUCTS, CONSTANTS = _read_header()
ConvDesc, NhwcConvDesc, H16ConvDesc = (_STRUCTS[n] for n in ("otp_conv_desc", "otp_nhwc_conv_desc", "otp_h16_conv_desc"))

OTP_OK = CONSTANTS["OTP_OK"]
_ERRORS = {CONSTANTS[name]: f"{name} ({text})" for name, text in (
    ("OTP_ERR_BAD_ARG", "null pointer or non-positive dimension"),
    ("OTP_ERR_UNSUPPORTED", "shape / dtype / stride combination not implemented"),
    ("OTP_ERR_LAUNCH", "HIP launch error"),
    ("OTP_ERR_WORKSPACE", "workspace too small"))}


def lib():
    """Return the loaded library, loading it on first use; raise loudly when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise RuntimeError(
                f"HIP library {LIB_PATH} is missing - run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C otpose_amd/csrc`). otpose_amd has no CPU or PyTorch-op fallback.")
        cdll = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(cdll, name)
            fn.restype = res
            fn.argtypes = args
        # one arithmetic switch for the whole library: OTPOSE_CONV_MATH=f32 keeps every product on the f32 MFMA
        cdll.otp_chan_attn_set_split(0 if os.environ.get("OTPOSE_CONV_MATH", "x3") == "f32" else 1)
        import torch
        if torch.cuda.is_available():
            cdll.otp_range_flag_read(0)       # allocates the range guard's pinned word now, outside any stream capture
        _lib = _DeviceGuarded(cdll)
    return _lib


class _DeviceGuarded:
    """The loaded library with every entry point wrapped so that a launch runs with the device of its tensors current:
    the kernels are enqueued on the stream ``stream_of(t)`` returned, and a HIP launch (and ``hipFuncSetAttribute``)
    applies to the *current* device.  PyTorch's current device is per thread and DataParallel-style callers already set
    it, so the guard only acts when a caller hands tensors of another device (single-process multi-device use)."""

    def __init__(self, cdll):
        self._cdll = cdll
        for name in SIGNATURES:
            setattr(self, name, self._wrap(getattr(cdll, name)))

    @staticmethod
    def _wrap(fn):
        import torch

        cur = getattr(torch._C, "_cuda_getDevice", None) or torch.cuda.current_device      # (the C call: no lazy-init check per launch)

        def call(*args):
            dev = getattr(_tls, "dev", None)
            if dev is not None and dev != cur():
                with torch.cuda.device(dev):
                    return fn(*args)
            return fn(*args)
        return call


def check(status: int, what: str):
    if status != OTP_OK:
        raise RuntimeError(f"{what} failed: {_ERRORS.get(status, status)}")


def ptr(t):
    """Device pointer of a tensor (``None`` -> NULL)."""
    return None if t is None else c_void_p(t.data_ptr())


def stream_of(t):
    """The HIP stream PyTorch is currently enqueuing on for ``t``'s device."""
    import torch
    dev = t.device.index
    _tls.dev = dev
    raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)     # the handle without building a torch.cuda.Stream object
    if raw is not None:                                              # (5 us per launch on the host-bound training forward)
        return c_void_p(raw(dev))
    return c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


_SIDE_STREAMS = {}            # device -> side streams shared by every inference engine and training graph of the process


def side_streams(device, n, first=0):
    """Side streams ``first`` .. ``first + n - 1`` of ``device`` from one process-wide pool (created on first use).
    The runtime multiplexes HIP streams onto a handful of hardware queues (four by default): an engine and a training graph
    that each created their own three would share queues and serialise branches that are meant to overlap (measured: the
    training step after two engines had been built ran 158 instead of 142 ms).  Engines and training steps of one process
    do not run concurrently, so they can share the streams."""
    import torch
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    pool = _SIDE_STREAMS.setdefault(device, [])
    while len(pool) < first + n:
        pool.append(torch.cuda.Stream(device))
    return pool[first:first + n]

