"""Build + load liblab4d_hip.so (the C-ABI in include/lab4d_hip.h) through ctypes.

No torch types cross the boundary: tensors are passed as raw device pointers, the stream as the
hipStream_t handle of torch's current stream.  There is NO fallback: if the shared library is
missing or a call fails, a RuntimeError is raised.
"""
import ctypes
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(ROOT, "include")
SO_PATH = os.environ.get("LAB4D_SO_PATH", os.path.join(HERE, "liblab4d_hip.so"))  # override: kernel experiments only
BUILD_DIR = os.environ.get("LAB4D_BUILD_DIR", os.path.join(HERE, "build"))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"
CFLAGS = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-I" + INCLUDE, "-I" + CSRC,
          "-Wno-unused-value", "-Wno-pass-failed"] + os.environ.get("LAB4D_HIPCC_EXTRA", "").split()
# (No -ffast-math and no relaxed fp64 division or square root here, ever: csrc/hd_math.hpp (sqrt_rn) and csrc/occvis_math.hpp (cell_axis_box)
# take the IEEE double root and quotient as given on the device, and the GPU suite holds the kernels word for word to g++'s.)


# the chain-kernel instantiation units only: LLVM's "unclustered high register pressure" rescheduling stage sinks the LDS reads of the shared
# weight groups next to the MFMAs that use them (exposed LDS latency in the one-wave-per-SIMD kernels); measured with it off, together with
# the conditional accumulator fence (mlp_kernels.hpp acc_fence_if): 739 vs 756 ms per step (profiles/r04_flag_variants.json)
MLP_INST_FLAGS = ["-mllvm", "-amdgpu-disable-unclustered-high-rp-reschedule"]


def sources():
    return sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))


def _newer(src, dst):
    if not os.path.exists(dst):
        return True
    t = os.path.getmtime(dst)
    deps = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    deps += [os.path.join(INCLUDE, f) for f in os.listdir(INCLUDE)]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True):
    """hipcc --offload-arch=gfx950 every csrc/*.hip, link liblab4d_hip.so in-tree."""
    if "amdgpu-mfma-vgpr-form" in os.environ.get("LAB4D_HIPCC_EXTRA", ""):
        # csrc/mlp_kernels.hpp acc_fence_if: the one-wave-per-SIMD chain kernels drop the MFMA -> inline-asm hazard fence because their accumulators live in
        # AGPRs (a compiler-visible v_accvgpr_read sits in between); with the MFMA results forced into VGPRs that is no longer true
        raise RuntimeError("LAB4D_HIPCC_EXTRA passes -amdgpu-mfma-vgpr-form: the chain kernels' accumulator hazard fence assumes AGPR accumulators")
    os.makedirs(BUILD_DIR, exist_ok=True)
    # The compile flags are part of the staleness key: an experiment build (-DLAB4D_ABL_* ...) in this BUILD_DIR followed by a
    # default build must not leave objects of the other flag set behind -- rebuilds are per object and mtime-based, and lab4d_build_flags()
    # only reports what runtime.hip's own object saw.  A stamp of the full flag set lives beside the objects; when it differs, everything is rebuilt.
    stamp_path = os.path.join(BUILD_DIR, "flags.stamp")
    stamp = "\n".join([HIPCC] + CFLAGS + ["--inst--"] + MLP_INST_FLAGS) + "\n"
    try:
        with open(stamp_path) as fh:
            stale_flags = fh.read() != stamp
    except OSError:
        stale_flags = True
    if stale_flags:
        force = True
        if os.path.exists(stamp_path):
            os.remove(stamp_path)  # (written again only after every object of the new flag set exists)
    jobs = []
    objs = []
    for f in sources():
        src = os.path.join(CSRC, f)
        obj = os.path.join(BUILD_DIR, f[:-4] + ".o")
        objs.append(obj)
        if force or _newer(src, obj):
            jobs.append((src, obj))

    def cc(job):
        src, obj = job
        inst = os.path.basename(src).startswith("mlp_inst_")
        cmd = [HIPCC] + CFLAGS + (MLP_INST_FLAGS if inst else []) + ["-c", src, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed for %s:\n%s" % (src, r.stderr[-4000:]))
        if verbose:
            print("[lab4d_amd] compiled", os.path.basename(src), file=sys.stderr)
        return obj

    if jobs:
        with ThreadPoolExecutor(max_workers=min(8, len(jobs))) as ex:
            list(ex.map(cc, jobs))
    if stale_flags:
        with open(stamp_path, "w") as fh:
            fh.write(stamp)
    if jobs or not os.path.exists(SO_PATH):
        cmd = [HIPCC, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", SO_PATH] + objs
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("link failed:\n%s" % r.stderr[-4000:])
        if verbose:
            print("[lab4d_amd] linked", SO_PATH, file=sys.stderr)
    return SO_PATH


_LIB = None
vp, ci = ctypes.c_void_p, ctypes.c_int

# The prototypes in include/*.h are the single source of the ctypes signatures: nothing on the Python side lists or counts arguments.
_SCALARS = {"int": ci, "int32_t": ci, "uint32_t": ctypes.c_uint32, "float": ctypes.c_float, "long": ctypes.c_long, "int64_t": ctypes.c_int64,
            "long long": ctypes.c_longlong}
_RETURNS = {"int": ci, "long": ctypes.c_long, "int64_t": ctypes.c_int64, "long long": ctypes.c_longlong, "const char*": ctypes.c_char_p}
_PROTOTYPE = re.compile(r"^[ \t]*([A-Za-z_][\w \t*]*?)\s*\b(lab4d_\w+)\s*\(([^()]*)\)\s*;", re.M)


def _declarations(text):
    """(return type, name, parameter text, the prototype on one line) of every `<return type> lab4d_<name>(<params>);` outside the comments."""
    for ret, name, params in _PROTOTYPE.findall(re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)):
        yield ret, name, params, "%s %s(%s)" % (ret.strip(), name, " ".join(params.split()))


def parse_parameters(params, where, proto):
    """The parameter text of one C function -> a list with a ctypes scalar type, c_void_p for a data pointer, or the C NAME of a lab4d_* struct
    for a pointer to one (argtypes() gives it its type).  A type outside _SCALARS raises: there is no default.  (The one copy of this rule:
    tests/host_twin.py reads the CPU twins' definitions with it.)"""
    args = []
    for p in [] if params.strip() in ("", "void") else params.split(","):
        words = [w for w in p.replace("*", " * ").split() if w != "const"]
        if "*" in words:
            args.append(words[0] if words[0].startswith("lab4d_") else vp)
        else:  # `<type> <name>` or a bare `<type>`
            key = " ".join(words) if " ".join(words) in _SCALARS else " ".join(words[:-1])
            if key not in _SCALARS:
                raise TypeError("%s: parameter '%s' of `%s` is neither a pointer nor one of %s" % (where, p.strip(), proto, sorted(_SCALARS)))
            args.append(_SCALARS[key])
    return args


def parse_prototypes(text, where):
    """C header text -> {name: (restype, params, has_stream)} for every `<return type> lab4d_<name>(<params>);` in it, the parameters as
    parse_parameters gives them.  A return type outside _RETURNS raises as well."""
    out = {}
    for ret, name, params, proto in _declarations(text):
        ret = re.sub(r"\s*\*", "*", " ".join(ret.split()))
        if ret not in _RETURNS:
            raise TypeError("%s: return type '%s' of `%s` is not one of %s" % (where, ret, proto, sorted(_RETURNS)))
        out[name] = (_RETURNS[ret], parse_parameters(params, where, proto), bool(re.search(r"\bstream\s*(,|$)", params)))
    return out


SIGNATURES = {}  # name -> (restype, params, has_stream) of every prototype in include/*.h
for _h in sorted(os.listdir(INCLUDE)):
    if _h.endswith(".h"):
        with open(os.path.join(INCLUDE, _h)) as _fh:
            SIGNATURES.update(parse_prototypes(_fh.read(), "include/" + _h))
MIRRORS = {}  # C struct name -> its ctypes.Structure mirror


def argtypes(params, mirrors=MIRRORS):
    """The ctypes argtypes of a parsed parameter list: a struct pointer is POINTER(mirror) once the mirror is bound, c_void_p until then (which
    takes no Structure: such a function cannot be called without the module that builds the struct)."""
    return [(ctypes.POINTER(mirrors[p]) if p in mirrors else vp) if isinstance(p, str) else p for p in params]


def mirrors(c_name):
    """Class decorator: binds a ctypes.Structure to the C struct it mirrors (tests/test_abi.py holds every bound mirror against a C compiler)."""
    def bind(cls):
        MIRRORS[c_name] = cls
        if _LIB is not None:
            for name, (_, params, _) in SIGNATURES.items():
                if c_name in params:
                    getattr(_LIB, name).argtypes = argtypes(params)
        return cls
    return bind


@mirrors("lab4d_field_list")
class FieldList(ctypes.Structure):
    _fields_ = [("n_fields", ci), ("fields", vp * 16), ("channels", ci * 16), ("modes", ci * 16)]


@mirrors("lab4d_field_grads")
class FieldGrads(ctypes.Structure):
    _fields_ = [("n_fields", ci), ("fields", vp * 16)]


def lib():
    """The loaded shared library.  Raises if it has not been built (no silent fallback)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(SO_PATH):
            raise RuntimeError(
                "liblab4d_hip.so is missing (%s). Build it with `python -c 'import __graft_entry__ as g; g.build()'`; "
                "lab4d_amd has no CPU or eager-PyTorch fallback." % SO_PATH)
        so = ctypes.CDLL(SO_PATH)
        for name, (restype, params, _) in SIGNATURES.items():
            fn = getattr(so, name)
            fn.restype, fn.argtypes = restype, argtypes(params)
        flags = so.lab4d_build_flags().decode().split()
        if flags and os.environ.get("LAB4D_ALLOW_EXPERIMENT_BUILD", "0") != "1":
            # kernel-experiment builds (tools/build_variants.sh) are loaded through LAB4D_SO_PATH by the timing tools only, which set the override
            raise RuntimeError("%s was compiled with kernel-experiment macros %s (most of them give wrong results); rebuild without them, or set "
                               "LAB4D_ALLOW_EXPERIMENT_BUILD=1 for a timing experiment" % (SO_PATH, flags))
        _LIB = so
    return _LIB if PROF is None else _ProfiledLib(_LIB)


class _ProfiledLib:
    """While per-kernel profiling is on (PROF is a dict): every entry point that launches (its prototype has a `stream` parameter) and is not
    already inside a `timed` block is timed under its own name, so the per-kernel table of the bench line accounts for ALL of the library's
    launches, not only the ones with a work model."""

    def __init__(self, lib_):
        self._lib = lib_

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if PROF is None or _TIMED_DEPTH > 0 or not SIGNATURES.get(name, (None, None, False))[2]:  # no stream parameter: host-only
            return fn

        def call(*a):
            with timed(name[6:]) as t:
                rc = fn(*a)
                t.on = t.on and rc == 0  # refused on the host: nothing was launched, nothing to time
            return rc
        return call


# LAB4D_NANCHECK=1 (diagnostic): every tensor whose pointer is handed to the library is remembered, and after each entry point returns
# the device is synchronised and the floating-point ones are scanned for non-finite values -- the first report names the kernel that
# produced (or was fed) them.  Together with torch.utils.deterministic.fill_uninitialized_memory (torch.empty -> NaN) this finds reads
# of uninitialised buffers.  Off by default: one attribute test per pointer.
NANCHECK = os.environ.get("LAB4D_NANCHECK", "0") == "1"
NANCHECK_IGNORE = set(os.environ.get("LAB4D_NANCHECK_IGNORE", "").split(","))
_SEEN = []
_REPORTED = set()


def _nancheck(what):
    torch.cuda.synchronize()
    for i, t in enumerate(_SEEN):
        if t.dtype.is_floating_point and t.numel() and what not in NANCHECK_IGNORE:
            flat = t.reshape(-1)
            n, first = 0, -1
            for o in range(0, flat.numel(), 1 << 28):  # pieces: index arithmetic of nonzero() overflows on > 2^31 elements
                piece = flat[o:o + (1 << 28)]
                bad = ~(piece.abs() < 1e15)  # non-finite, or a magnitude no quantity of this renderer reaches (uninitialised memory)
                k = int(bad.sum())
                if k and first < 0:
                    first = o + int(bad.to(torch.uint8).argmax())
                n += k
            if n and n < t.numel() and (what, i) not in _REPORTED:  # a buffer that is ALL poison has simply not been written yet
                _REPORTED.add((what, i))
                print("[nancheck] %s: tensor #%d %s %s has %d non-finite / huge values of %d (first at flat index %d: %s)"
                      % (what, i, tuple(t.shape), str(t.dtype).replace("torch.", ""), n, t.numel(), first, float(flat[first])), file=sys.stderr)
    _SEEN.clear()


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed (%d): %s" % (what, rc, lib().lab4d_last_error().decode()))
    if NANCHECK:
        _nancheck(what)


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    if NANCHECK:
        _SEEN.append(t)
    return ctypes.c_void_p(t.data_ptr())


def dp(t):
    """Raw device address of a tensor, for pointer fields of the argument structs."""
    if NANCHECK:
        _SEEN.append(t)
    return t.data_ptr()


def ptr_at(t):
    """Device pointer of the first element of a (possibly non-contiguous) view; the caller passes the row stride."""
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


DTYPE_CODE = {torch.float32: 0, torch.float16: 1, torch.float64: 2}


def require_device(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("lab4d_amd ops need device (HIP) tensors; got a %s tensor -- there is no CPU path" % t.device)
        if not t.is_contiguous():
            raise RuntimeError("lab4d_amd ops need contiguous tensors")


def prototype(full):
    """The C prototype of an entry point on one line, as include/*.h declares it (for error messages)."""
    for h in sorted(os.listdir(INCLUDE)):
        if h.endswith(".h"):
            with open(os.path.join(INCLUDE, h)) as fh:
                for _, name, _, proto in _declarations(fh.read()):
                    if name == full:
                        return proto


_BYREF = type(ctypes.byref(ci()))
_STRUCT_POINTERS = (ctypes._Pointer, _BYREF)
_DATA_POINTERS = (vp, ctypes.Array) + _STRUCT_POINTERS  # what a data-pointer slot takes beside None and a tensor


def marshal(name, args):
    """The ctypes-ready values of `args` for the entry point lab4d_<name>, each held against its slot of the parsed prototype (the stream is not
    among them).  A data pointer takes None, a contiguous device tensor or a ctypes pointer/array -- never a number, which c_void_p would pass
    on as an address; a struct pointer takes None, the bound mirror or a byref/pointer; an integer slot an int; a float slot an int or a float.
    Decided by include/*.h alone: the library is not touched."""
    full = "lab4d_" + name
    if full not in SIGNATURES:
        raise RuntimeError("include/*.h declares no entry point %s" % full)
    _, params, has_stream = SIGNATURES[full]
    if len(args) != len(params) - has_stream:
        raise TypeError("%s takes %d arguments%s, got %d: `%s`"
                        % (full, len(params) - has_stream, " before the stream" if has_stream else "", len(args), prototype(full)))

    def refuse(i, wants):
        got = "a %s tensor" % str(args[i].dtype).replace("torch.", "") if isinstance(args[i], torch.Tensor) else repr(args[i])
        return TypeError("%s: args[%d] must be %s, got %s: `%s`" % (full, i, wants, got, prototype(full)))

    out = []
    for i, (p, a) in enumerate(zip(params, args)):
        if p is vp:
            if isinstance(a, torch.Tensor):
                if not (a.is_cuda and a.is_contiguous()):
                    require_device(a)  # (raises; not called on the good path: it costs as much as the rest of the slot)
                a = ptr(a)
            elif a is not None and not isinstance(a, _DATA_POINTERS):
                raise refuse(i, "a data pointer (None, a device tensor or a ctypes pointer)")
        elif isinstance(p, str):
            if isinstance(a, MIRRORS.get(p, ())):
                a = ctypes.byref(a)
            elif a is not None and not isinstance(a, _STRUCT_POINTERS):
                raise refuse(i, "a pointer to %s (None, its ctypes mirror or a byref of one)" % p)
        elif p is ctypes.c_float:
            if not isinstance(a, (int, float)):
                raise refuse(i, "a number")
        elif not isinstance(a, int):
            raise refuse(i, "an int")
        out.append(a)
    return out


def call(name, *args, what=None):
    """Launch the status-returning entry point lab4d_<name>: marshal() the arguments, add torch's current stream where the prototype has one,
    and raise on a non-zero status (labelled `what`, by default the name)."""
    a = marshal(name, args)
    if SIGNATURES["lab4d_" + name][2]:
        a.append(stream())
    check(getattr(lib(), "lab4d_" + name)(*a), what or name)


# --------------------------------------------------------------------------------------------------
# optional per-kernel-family timing with HIP events on the launch stream (used by bench.py's roofline)
# --------------------------------------------------------------------------------------------------
_TIMED_DEPTH = 0
PROF = None  # set to {} to enable: name -> list of (start_event, end_event, work)


class timed:
    """`with timed("mlp_fwd_base", flops): launch...` records HIP events around the launches on torch's
    current stream (the stream the kernels are launched on)."""

    def __init__(self, name, work=0.0):
        self.name, self.work = name, work

    def __enter__(self):
        global _TIMED_DEPTH
        _TIMED_DEPTH += 1
        self.on = PROF is not None and _TIMED_DEPTH == 1  # nested blocks belong to the outer one
        if self.on:
            self.s = torch.cuda.Event(enable_timing=True)
            self.e = torch.cuda.Event(enable_timing=True)
            self.s.record()
        return self

    def __exit__(self, exc_type, *a):
        global _TIMED_DEPTH
        _TIMED_DEPTH -= 1
        if self.on and PROF is not None and exc_type is None:  # (a block that raised -- an entry point refused its arguments -- is no launch)
            self.e.record()
            PROF.setdefault(self.name, []).append((self.s, self.e, self.work))
        return False


def prof_summary():
    """name -> (launches, total_ms, total_flops, total_bytes). Call after torch.cuda.synchronize()."""
    out = {}
    for k, v in (PROF or {}).items():
        fl = sum((w[0] if isinstance(w, tuple) else w) for _, _, w in v)
        by = sum((w[1] if isinstance(w, tuple) else 0.0) for _, _, w in v)
        out[k] = (len(v), sum(s.elapsed_time(e) for s, e, _ in v), fl, by)
    return out
