"""The one builder of the CPU twins (tests/host_harness/<name>_host.cpp over lab4d_amd/csrc/<name>_math.hpp) and of what else the harness
compiles: load() builds a twin with g++ and sets restype / argtypes of every extern "C" function from the source text, by the parameter rule
of lab4d_amd/_lib.py; sanitized_main() builds a twin's stand-alone program under the sanitizers; kernel_metadata() reads the code-object
metadata of one csrc/*.hip.  A helper module: no test, no conftest."""
import ctypes
import functools
import os
import re
import subprocess

from lab4d_amd import _lib

HARNESS = os.path.join(_lib.ROOT, "tests", "host_harness")
BUILD = os.path.join(HARNESS, "_build")
_RETURNS = {"int": ctypes.c_int, "void": None, "float": ctypes.c_float}
_DEFINITION = re.compile(r'extern\s+"C"\s+([A-Za-z_][\w \t*]*?)\s*\b(\w+)\s*\(([^()]*)\)\s*\{')


def signatures(text, where):
    """C++ source text -> {name: (restype, argtypes)} of every `extern "C" <return type> <name>(<params>) {` outside the comments.  A type
    outside the closed maps (_RETURNS here, _lib._SCALARS) raises: there is no default."""
    out = {}
    for ret, name, params in _DEFINITION.findall(re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)):
        proto = "%s %s(%s)" % (ret, name, " ".join(params.split()))
        if ret not in _RETURNS:
            raise TypeError("%s: return type '%s' of `%s` is not one of %s" % (where, ret, proto, sorted(_RETURNS)))
        out[name] = (_RETURNS[ret], _lib.parse_parameters(params, where, proto))
    return out


def _gxx(flags, src, out):
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++"] + flags + [os.path.join(HARNESS, src), "-o", os.path.join(BUILD, out)])
    return os.path.join(BUILD, out)


@functools.lru_cache(None)
def load(name):
    """The twin <name>_host.cpp as a ctypes library, every function typed.  Compiled on first use in a process (never stale against its
    header), then shared."""
    src = name + "_host.cpp"
    lib = ctypes.CDLL(_gxx(["-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", _lib.CSRC], src, name + "_host.so"))
    with open(os.path.join(HARNESS, src)) as fh:
        for fn, (restype, argtypes) in signatures(fh.read(), "tests/host_harness/" + src).items():
            f = getattr(lib, fn)
            f.restype, f.argtypes = restype, argtypes
    return lib


def sanitized_main(name):
    """<name>_host_main.cpp with AddressSanitizer and UndefinedBehaviorSanitizer: the path of a stand-alone program, to be run as a child
    process (the runtimes are linked statically: the program needs nothing from its environment)"""
    return _gxx(["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all",
                 "-fno-omit-frame-pointer", "-I", _lib.CSRC, "-I", HARNESS], name + "_host_main.cpp", name + "_host_main_asan")


_METADATA = ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count", "agpr_count")


def kernel_metadata(hip_file, tmp_path):
    """csrc/<hip_file> compiled for gfx950 as the build does: one dict per kernel of the code-object metadata, `name` and the integers of
    _METADATA (vgpr_count is the unified count: AGPRs included)."""
    subprocess.check_call([_lib.HIPCC] + _lib.CFLAGS + ["-save-temps=obj", "-c", os.path.join(_lib.CSRC, hip_file), "-o", str(tmp_path / "kernels.o")])
    asm = [f for f in os.listdir(tmp_path) if f.endswith(".s") and "amdgcn" in f]
    assert len(asm) == 1, asm
    kernels, = re.findall(r"^amdhsa\.kernels:\n((?: .*\n)+)", open(tmp_path / asm[0]).read(), flags=re.M)  # (the indented lines below the key)
    out = []
    for entry in re.split(r"^  - ", kernels, flags=re.M)[1:]:  # a kernel's own keys: at the entry's indent, its arguments' lie deeper
        keys = dict(re.findall(r"^(?:    )?\.(\w+):[ \t]+(\S+)$", entry, flags=re.M))
        out.append(dict({k: int(keys[k]) for k in _METADATA}, name=keys["name"]))
    return out
