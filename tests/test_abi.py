"""CPU-only checks of the drop-in boundary: the C-ABI library builds for gfx950, loads, and exports
every symbol that include/*.h declares (no compute calls -- there is no GPU here)."""
import ctypes
import os
import re

import pytest

from lab4d_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    names = []
    for f in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if not f.endswith(".h"):
            continue
        src = open(os.path.join(ROOT, "include", f)).read()
        src = re.sub(r"/\*.*?\*/|//[^\n]*", "", src, flags=re.S)
        names += re.findall(r"\b(lab4d_[a-z0-9_]+)\s*\(", src)
    return sorted(set(names))


@pytest.fixture(scope="module")
def so():
    _lib.build(verbose=False)
    return ctypes.CDLL(_lib.SO_PATH)


def test_library_exports_every_declared_symbol(so):
    names = declared_symbols()
    assert len(names) >= 29
    missing = [n for n in names if not hasattr(so, n)]
    assert not missing, missing


def test_parser_skips_no_prototype(so):
    """The ctypes signatures are parsed from include/*.h (_lib.parse_prototypes): the strict prototype pattern finds exactly the names the loose
    `lab4d_*(` search above finds -- a prototype the parser cannot read is not silently left without argtypes -- and each resolves in the library."""
    assert sorted(_lib.SIGNATURES) == declared_symbols()
    assert not [n for n in _lib.SIGNATURES if not hasattr(so, n)]


SMALL_HEADER = """
/* a block comment that holds int lab4d_x(int a); and spans
   two lines */
// a line comment: int lab4d_y(int a);
typedef struct { int n; } lab4d_t;
int lab4d_three_lines(const float* x,   /* in */
                      unsigned char* mask, const int64_t* ids,
                      int n, void* stream);
long long lab4d_size(int a, long long b);
const char* lab4d_name(void);
int lab4d_takes(const lab4d_t* t, uint32_t k, void* stream);
"""


def test_parser_on_a_small_header():
    vp, ci = ctypes.c_void_p, ctypes.c_int
    sig = _lib.parse_prototypes(SMALL_HEADER, "small.h")
    assert sorted(sig) == ["lab4d_name", "lab4d_size", "lab4d_takes", "lab4d_three_lines"]  # nothing from inside the comments
    assert sig["lab4d_three_lines"] == (ci, [vp, vp, vp, ci, vp], True)
    assert sig["lab4d_size"] == (ctypes.c_longlong, [ci, ctypes.c_longlong], False)
    assert sig["lab4d_name"] == (ctypes.c_char_p, [], False)
    restype, params, has_stream = sig["lab4d_takes"]
    assert (restype, params, has_stream) == (ci, ["lab4d_t", ctypes.c_uint32, vp], True)

    class T(ctypes.Structure):
        _fields_ = [("n", ci)]
    assert _lib.argtypes(params, {}) == [vp, ctypes.c_uint32, vp]  # unbound: a plain pointer, which takes no Structure
    assert _lib.argtypes(params, {"lab4d_t": T}) == [ctypes.POINTER(T), ctypes.c_uint32, vp]
    with pytest.raises(TypeError):
        vp.from_param(T())
    with pytest.raises(TypeError, match=r"small\.h.*size_t n.*lab4d_bad"):
        _lib.parse_prototypes("int lab4d_bad(const float* x, size_t n, void* stream);", "small.h")
    with pytest.raises(TypeError, match=r"small\.h.*double.*lab4d_bad"):
        _lib.parse_prototypes("double lab4d_bad(void);", "small.h")


def test_pinned_signatures():
    """One signature per feature of the parser, written out by hand."""
    from lab4d_amd import mlp, packed  # noqa: F401  (mlp binds the mirror of lab4d_mlp_fwd_args)
    vp, ci, cu, cl, cf, i64, P = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_long, ctypes.c_float, ctypes.c_int64, ctypes.POINTER
    pinned = {
        "lab4d_quaternion_mul_forward": (ci, [vp, vp, vp, cu, cu, cu, ci, vp], True),
        "lab4d_occgrid_mask": (ci, [vp, vp, vp, ci, cl, vp, vp], True),
        "lab4d_adamw_step": (ci, [vp, vp, vp, vp, i64, vp, vp, ci, cf, cf, cf, cf, ci, vp, vp], True),
        "lab4d_skin_blend_backward_workspace_floats": (ctypes.c_longlong, [ci] * 5, False),
        "lab4d_mlp_forward": (ci, [P(mlp.FwdArgs), vp], True),
        "lab4d_packed_composite_backward": (ci, [vp, vp, P(_lib.FieldList), vp, vp, cl, cl, vp, vp, vp, vp, P(_lib.FieldGrads), vp], True),
    }
    for name, want in pinned.items():
        restype, params, has_stream = _lib.SIGNATURES[name]
        assert (restype, _lib.argtypes(params), has_stream) == want, name


def test_loaded_library_enforces_the_signatures(so):
    """lib() applies the parsed table to every function: a call one argument short is a TypeError before the library is entered, and a mirror
    bound after the load reaches the functions already set up."""
    L = _lib.lib()
    with pytest.raises(TypeError):
        L.lab4d_quaternion_conjugate(None, 1, None, 0)
    assert L.lab4d_last_error.restype is ctypes.c_char_p and list(L.lab4d_version.argtypes) == []
    old = _lib.MIRRORS["lab4d_field_list"]

    class Other(ctypes.Structure):
        _fields_ = old._fields_
    try:
        _lib.mirrors("lab4d_field_list")(Other)
        assert L.lab4d_composite_forward.argtypes[2] is ctypes.POINTER(Other)
    finally:
        _lib.mirrors("lab4d_field_list")(old)
    assert L.lab4d_composite_forward.argtypes[2] is L.lab4d_packed_composite_backward.argtypes[2] is ctypes.POINTER(old)


def test_data_pointer_parameters_take_host_arrays():
    """`const float* weights` of lab4d_ray_losses_* and `int* stats` of lab4d_mesh_largest_component are plain pointers (c_void_p): the host arrays
    their callers pass are accepted, with byref (deformable.RayLosses) and without (mesh.largest_component)."""
    for name, at in (("lab4d_ray_losses_forward", 3), ("lab4d_ray_losses_backward", 3), ("lab4d_mesh_largest_component", 8)):
        assert _lib.SIGNATURES[name][1][at] is ctypes.c_void_p
    w, stats = (ctypes.c_float * 12)(), (ctypes.c_int * 2)()
    for arg in (w, ctypes.byref(w), stats, None):
        ctypes.c_void_p.from_param(arg)


def good_args(name):
    """One valid argument per slot of lab4d_<name> (the stream left out): NULL for a pointer, 1 for an integer, 0.5 for a float."""
    _, params, has_stream = _lib.SIGNATURES["lab4d_" + name]
    return [0.5 if p is ctypes.c_float else None if p is ctypes.c_void_p or isinstance(p, str) else 1 for p in params[:len(params) - has_stream]]


@pytest.mark.parametrize("name,n_args,pointer_at,int_at,float_at", [("hashsdf_forward", 13, 1, 3, None), ("adamw_step", 14, 2, 4, 8)])
def test_marshal_checks_every_slot_against_the_prototype(name, n_args, pointer_at, int_at, float_at):
    """_lib.marshal (the argument half of _lib.call) decides by include/*.h alone -- no library, no GPU: the count, a number where a pointer
    belongs (c_void_p would pass it on as an address), a float or a tensor where an integer belongs, a host or strided tensor."""
    import torch
    good = good_args(name)
    assert len(good) == n_args
    out = _lib.marshal(name, good)
    assert out == good and len(out) == len(_lib.SIGNATURES["lab4d_" + name][1]) - 1  # (the stream is call()'s to add)
    proto = re.escape(_lib.prototype("lab4d_" + name))
    assert proto.startswith("int\\ lab4d_" + name) and "stream" in proto
    for bad in (good[:-1], good + [None]):
        with pytest.raises(TypeError, match="takes %d arguments.*got %d.*%s" % (n_args, len(bad), proto)):
            _lib.marshal(name, bad)

    def put(at, value):
        return good[:at] + [value] + good[at + 1:]
    for number in (4096, 1.0, True):
        with pytest.raises(TypeError, match=r"lab4d_%s: args\[%d\] must be a data pointer.*%s" % (name, pointer_at, proto)):
            _lib.marshal(name, put(pointer_at, number))
    with pytest.raises(TypeError, match=r"lab4d_%s: args\[%d\] must be an int" % (name, int_at)):
        _lib.marshal(name, put(int_at, 2.0))
    assert _lib.marshal(name, put(int_at, True))[int_at] is True
    with pytest.raises(RuntimeError, match="got a cpu tensor -- there is no CPU path"):
        _lib.marshal(name, put(pointer_at, torch.zeros(4)))
    with pytest.raises(RuntimeError, match="no CPU path"):
        _lib.marshal(name, put(pointer_at, torch.zeros(4, 2)[:, 0]))
    with pytest.raises(TypeError, match=r"args\[%d\] must be an int, got a int64 tensor" % int_at):  # (a 0-dim tensor here would be a hidden sync)
        _lib.marshal(name, put(int_at, torch.tensor(3)))
    if float_at is not None:
        assert _lib.marshal(name, put(float_at, 2))[float_at] == 2
        with pytest.raises(TypeError, match=r"args\[%d\] must be a number" % float_at):
            _lib.marshal(name, put(float_at, torch.tensor(0.5)))
    for host in (ctypes.c_void_p(64), (ctypes.c_float * 4)(), ctypes.byref(ctypes.c_int(0))):
        assert _lib.marshal(name, put(pointer_at, host))[pointer_at] is host
    with pytest.raises(RuntimeError, match="no entry point lab4d_%s_nope" % name):
        _lib.marshal(name + "_nope", good)


def test_marshal_takes_only_the_bound_mirror_in_a_struct_slot():
    name, at = "packed_composite_backward", 2
    assert _lib.SIGNATURES["lab4d_" + name][1][at] == "lab4d_field_list"
    good = good_args(name)
    fl = _lib.FieldList()
    for ok in (fl, ctypes.byref(fl), ctypes.pointer(fl)):
        ctypes.POINTER(_lib.FieldList).from_param(_lib.marshal(name, good[:at] + [ok] + good[at + 1:])[at])
    for bad in (_lib.FieldGrads(), 64, ctypes.c_void_p(64)):
        with pytest.raises(TypeError, match=r"args\[2\] must be a pointer to lab4d_field_list"):
            _lib.marshal(name, good[:at] + [bad] + good[at + 1:])


def test_every_call_site_names_a_prototype_and_counts_its_arguments():
    """Census of the package's launch sites, without a GPU: every _lib.call("<name>", ...) names an entry point of include/*.h and, where it
    spreads no list into the arguments, passes as many as the prototype has in front of its stream."""
    import ast
    sites = []
    for dirpath, _, files in os.walk(os.path.join(ROOT, "lab4d_amd")):
        for f in files:
            if not f.endswith(".py"):
                continue
            path = os.path.join(dirpath, f)
            for node in ast.walk(ast.parse(open(path).read())):
                if (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "call"
                        and isinstance(node.func.value, ast.Name) and node.func.value.id == "_lib"):
                    first = node.args[0]
                    names = [first] if isinstance(first, ast.Constant) else [first.body, first.orelse] if isinstance(first, ast.IfExp) else []
                    assert names and all(isinstance(n, ast.Constant) and isinstance(n.value, str) for n in names), (path, node.lineno)
                    sites += [(os.path.relpath(path, ROOT), node.lineno, n.value, node.args[1:]) for n in names]
    assert len(sites) >= 85, len(sites)
    for where, line, name, args in sites:
        assert "lab4d_" + name in _lib.SIGNATURES, (where, line, name)
        _, params, has_stream = _lib.SIGNATURES["lab4d_" + name]
        if not any(isinstance(a, ast.Starred) for a in args):
            assert len(args) == len(params) - has_stream, (where, line, name, _lib.prototype("lab4d_" + name))


def test_timed_entry_points_are_the_ones_with_a_stream(so):
    """_ProfiledLib times a function iff its prototype has a `stream` parameter: no size query, no getter."""
    timed_names = set()
    _lib.PROF = {}
    try:
        prof = _lib._ProfiledLib(so)
        for n in _lib.SIGNATURES:
            if getattr(prof, n) is not getattr(so, n):
                timed_names.add(n)
    finally:
        _lib.PROF = None
    assert timed_names == {n for n, (_, _, has_stream) in _lib.SIGNATURES.items() if has_stream}
    host_only = {"lab4d_last_error", "lab4d_arch", "lab4d_build_flags", "lab4d_version", "lab4d_mlp_fused_backward_supported", "lab4d_mlp_describe",
                 "lab4d_mlp_packed_bytes", "lab4d_compact_work_ints", "lab4d_global_match_workspace_floats",
                 "lab4d_skin_blend_backward_workspace_floats", "lab4d_mesh_work_ints", "lab4d_mesh_component_work_ints"}
    assert set(_lib.SIGNATURES) - timed_names == host_only


def test_library_targets_gfx950(so):
    so.lab4d_arch.restype = ctypes.c_char_p
    assert so.lab4d_arch() == b"gfx950"
    assert so.lab4d_version() >= 1


def test_shipped_library_has_no_experiment_macros(so):
    """csrc/ keeps exactly two compile-time experiment switches, LAB4D_WSABL_NOST and LAB4D_ABL_WGRAD_L2 (timing ablations that give wrong results,
    DESIGN.md section 8): the library the product loads must have been compiled with neither, the LAB4D_* macros the sources test must be exactly
    these two (no new ones grow back), and lab4d_build_flags() must report exactly them."""
    import re
    so.lab4d_build_flags.restype = ctypes.c_char_p
    assert so.lab4d_build_flags() == b"", so.lab4d_build_flags()
    csrc = os.path.join(ROOT, "lab4d_amd", "csrc")
    tested = set()
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".hpp")):
            src = open(os.path.join(csrc, f)).read()
            tested |= set(re.findall(r"#\s*ifn?def\s+(LAB4D_[A-Z0-9_]+)", src)) | set(re.findall(r"defined\s*\(?\s*(LAB4D_[A-Z0-9_]+)", src))
            tested |= set(re.findall(r"#\s*(?:el)?if\b[^\n]*?\b(LAB4D_[A-Z0-9_]+)", src))
    tested -= {"LAB4D_HIP_H"}
    assert tested == {"LAB4D_WSABL_NOST", "LAB4D_ABL_WGRAD_L2"}, sorted(tested)
    runtime = open(os.path.join(csrc, "runtime.hip")).read()
    reported = set(re.findall(r"#ifdef (LAB4D_[A-Z0-9_]+)", runtime))
    assert tested == reported, (sorted(tested), sorted(reported))


def test_bad_arguments_are_rejected_without_a_gpu(so):
    # argument validation happens before any launch, so it is testable on CPU
    so.lab4d_last_error.restype = ctypes.c_char_p
    rc = so.lab4d_quaternion_mul_forward(None, None, None, 4, 4, 4, 0, None)
    assert rc == -1 and b"null" in so.lab4d_last_error()
    buf = ctypes.create_string_buffer(64)
    rc = so.lab4d_quaternion_mul_forward(buf, buf, buf, ctypes.c_uint32(1), ctypes.c_uint32(5), ctypes.c_uint32(4), 0, None)
    assert rc == -1 and b"3 or 4" in so.lab4d_last_error()
    rc = so.lab4d_quaternion_conjugate(buf, ctypes.c_uint32(1), buf, 9, None)
    assert rc == -1 and b"dtype" in so.lab4d_last_error()


def test_ops_refuse_cpu_tensors():
    import torch
    from lab4d_amd import quaternion
    with pytest.raises(RuntimeError, match="no CPU path"):
        quaternion.quaternion_mul(torch.randn(3, 4), torch.randn(3, 4))


def test_fk_arguments_are_validated(so):
    so.lab4d_last_error.restype = ctypes.c_char_p
    buf = ctypes.create_string_buffer(64)
    rc = so.lab4d_fk_forward(buf, buf, None, buf, buf, 1, 33, 0, buf, buf, None)
    assert rc == -1 and b"B <= 32" in so.lab4d_last_error()
    rc = so.lab4d_skel_bones_forward(buf, None, buf, buf, buf, buf, buf, buf, 1, 25, buf, buf, None)
    assert rc == -1 and b"null" in so.lab4d_last_error()
    assert so.lab4d_fk_forward(buf, buf, None, buf, buf, 0, 25, 0, buf, buf, None) == 0  # empty input: nothing to launch


def test_pose_refuses_cpu_tensors():
    import torch
    from lab4d_amd import pose
    with pytest.raises(RuntimeError, match="no CPU path"):
        pose.fk_se3(torch.zeros(2, 3, 3), torch.zeros(2, 3, 3), {1: 0, 2: 1, 3: 2})


def test_product_package_never_imports_the_oracle():
    """oracle/ is test infrastructure: only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import it."""
    import ast
    pkg = os.path.join(ROOT, "lab4d_amd")
    offenders = []
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if not f.endswith(".py"):
                continue
            tree = ast.parse(open(os.path.join(dirpath, f)).read())
            for node in ast.walk(tree):
                names = []
                if isinstance(node, ast.Import):
                    names = [a.name for a in node.names]
                elif isinstance(node, ast.ImportFrom):
                    names = [node.module or ""]
                if any(n == "oracle" or n.startswith("oracle.") for n in names):
                    offenders.append(os.path.join(dirpath, f))
    assert not offenders, offenders
    # bench.py: the oracle is imported inside cpu_baseline() only
    tree = ast.parse(open(os.path.join(ROOT, "bench.py")).read())
    for fn in [n for n in tree.body if isinstance(n, ast.FunctionDef)]:
        uses = any(isinstance(n, ast.ImportFrom) and (n.module or "").startswith("oracle") for n in ast.walk(fn))
        assert uses == (fn.name == "cpu_baseline"), fn.name
    assert not any(isinstance(n, (ast.Import, ast.ImportFrom)) and "oracle" in ast.dump(n) for n in tree.body)


def test_rowmlp_programs_are_validated_before_any_launch(so):
    """include/lab4d_rowmlp.h's contract on the CPU (argument checks run before the launch): a layer writing into its own input, two layers writing
    overlapping columns, columns leaving the strip, too many layers -- all refused with LAB4D_EINVAL and a message."""
    from lab4d_amd import rowmlp
    so.lab4d_last_error.restype = ctypes.c_char_p
    so.lab4d_rowmlp_forward.argtypes = [ctypes.POINTER(rowmlp._Prog), ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]

    def prog(layers, stride=64):
        p = rowmlp._Prog()
        p.n_layers, p.row_stride = len(layers), stride
        for i, (i_dim, o_dim, src, dst) in enumerate(layers):
            q = p.layer[i]
            q.W, q.in_dim, q.out_dim, q.src_col, q.dst_col = 0x1000, i_dim, o_dim, src, dst  # (never dereferenced: the checks fail first)
        return p

    fake = ctypes.c_void_p(0x2000)
    for layers, word in [([(8, 8, 0, 4)], b"own input"), ([(8, 8, 0, 16), (8, 8, 16, 20)], b"own input"), ([(8, 8, 0, 16), (8, 8, 0, 20)], b"overlapping"),
                         ([(8, 8, 0, 60)], b"leave the row strip"), ([(2000, 8, 0, 16)], b"outside")]:
        p = prog(layers, stride=64 if layers[0][0] < 100 else 4096)
        assert so.lab4d_rowmlp_forward(ctypes.byref(p), fake, 4, None) == -1
        assert word in so.lab4d_last_error(), (layers, so.lab4d_last_error())
    p = prog([(8, 8, 0, 16)])
    p.n_layers = 17
    assert so.lab4d_rowmlp_forward(ctypes.byref(p), fake, 4, None) == -1


def c_struct_fields():
    """C struct name -> its field names in declaration order, for every `typedef struct {...} lab4d_*;` of include/*.h."""
    out = {}
    for f in sorted(os.listdir(os.path.join(ROOT, "include"))):
        src = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(os.path.join(ROOT, "include", f)).read(), flags=re.S)
        for body, name in re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*(lab4d_\w+)\s*;", src, flags=re.S):
            pieces = [p.strip() for decl in body.split(";") for p in decl.split(",")]  # `const float *mask, *feature;` declares two fields
            out[name] = [re.search(r"(\w+)\s*(\[[^\]]*\])?$", p).group(1) for p in pieces if p]
    return out


def test_ctypes_structs_have_the_c_layout(tmp_path):
    """Every ctypes.Structure that mirrors a struct of include/*.h (bound with _lib.mirrors: the nine argument structs and the three nested in
    them) has the layout a C compiler gives the header: the same fields by name in the same order, and for each the same offset and size, and
    the same total size (a field added on one side only would shift every pointer behind it).  No struct of the headers is left without a mirror."""
    import subprocess
    from lab4d_amd import deformable, mlp, rowmlp
    py_name = {"in": "inp"}  # `in` is a Python keyword
    c_fields = c_struct_fields()
    assert _lib.MIRRORS == {
        "lab4d_field_list": _lib.FieldList, "lab4d_field_grads": _lib.FieldGrads, "lab4d_mlp_layer": mlp.LayerDesc, "lab4d_mlp_desc": mlp.NetDesc,
        "lab4d_mlp_fwd_args": mlp.FwdArgs, "lab4d_mlp_bwd_args": mlp.BwdArgs, "lab4d_mlp_bwd_fused_args": mlp.BwdFusedArgs,
        "lab4d_loss_inputs": deformable._LossInputs, "lab4d_loss_grads": deformable._LossGrads, "lab4d_rowmlp_layer": rowmlp._Layer,
        "lab4d_rowmlp_io": rowmlp._IO, "lab4d_rowmlp_prog": rowmlp._Prog}
    assert set(c_fields) == set(_lib.MIRRORS)
    assert {p for _, params, _ in _lib.SIGNATURES.values() for p in params if isinstance(p, str)} <= set(_lib.MIRRORS)
    headers = sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h"))
    lines = []
    for name, fields in c_fields.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        lines += ['printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (name, f, name, f, name, f) for f in fields]
    src = tmp_path / "sz.c"
    src.write_text("#include <stdint.h>\n#include <stddef.h>\n#include <stdio.h>\n" + "".join('#include "%s"\n' % h for h in headers)
                   + "int main(void){\n" + "\n".join(lines) + "\nreturn 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    c = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        key, *nums = line.split()
        c[key] = [int(x) for x in nums]
    for name, cls in _lib.MIRRORS.items():
        assert [n for n, _ in cls._fields_] == [py_name.get(f, f) for f in c_fields[name]], name
        assert c[name] == [ctypes.sizeof(cls)], name
        for f in c_fields[name]:
            d = getattr(cls, py_name.get(f, f))
            assert c[name + "." + f] == [d.offset, d.size], (name, f)
    # the sizes the entry points' argument structs have today (include/*.h at this commit)
    assert [c[n][0] for n in ("lab4d_field_list", "lab4d_field_grads", "lab4d_mlp_desc", "lab4d_mlp_fwd_args", "lab4d_mlp_bwd_args",
                              "lab4d_mlp_bwd_fused_args", "lab4d_loss_inputs", "lab4d_loss_grads", "lab4d_rowmlp_prog")] == \
        [264, 136, 412, 576, 488, 736, 208, 112, 1120]
