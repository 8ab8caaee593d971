"""CPU-side checks of the C-ABI library: ``lvdgs._abi`` -- every struct, constant and prototype -- agrees with include/lvdgs.h
as gcc reads it, the library loads and exports every symbol the header declares, and argument validation works without
touching a GPU."""
import copy
import ctypes as C
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import pytest

from lvdgs import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lvdgs.h")


# ---------------------------------------------------------------- the mirror against the header
# Upper-case integers of _abi that are no LVDGS_* name of the header: name -> (words of the header line it restates, value)
RESTATED = {
    "TSDF_OVERFLOW_VERTICES": ("[_OVERFLOW] bit 0: more vertices than vertex_capacity", 1 << 0),
    "TSDF_OVERFLOW_FACES": ("more faces than face_capacity", 1 << 1),
    "TSDF_OVERFLOW_INT32": ("more faces than face_capacity, bit 2: more than 2^31 - 1 faces", 1 << 2),
    "MAP_OUTSIDE": ('stored as INT32_MIN and means "outside"', -2 ** 31),
    "FRAME_EVAL_ROW_BYTES": ("The row (64 bytes, written by the finishing launch", 64),
}

SCALARS = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "uint8_t": C.c_uint8,
           "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "int": C.c_int, "char": C.c_char}

# the kind of a struct field as C sees it: signed / unsigned integer, floating, char, anything else (a pointer: arrays decay)
KIND = ('#define KIND(x) _Generic((x), signed char: "i", short: "i", int: "i", long: "i", long long: "i", '
        'unsigned char: "u", unsigned short: "u", unsigned: "u", unsigned long: "u", unsigned long long: "u", '
        'float: "f", double: "f", char: "c", default: "p")')


def mirror_of(module):
    """What a module such as _abi states, as the plain data ``mismatches`` reads: structs by C name, integers by name, prototypes."""
    classes = [v for v in vars(module).values() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure]
    return SimpleNamespace(structs={getattr(c, "_c_name_", c.__name__): c for c in classes},
                           constants={n: v for n, v in vars(module).items() if n.isupper() and type(v) is int},
                           prototypes=dict(module.PROTOTYPES))


def ctype_kind(t):
    if issubclass(t, (C.Array, C.Structure)):
        return "-"      # compared by offset and size
    if issubclass(t, C._Pointer) or t in (C.c_void_p, C.c_char_p):
        return "p"
    return {**dict.fromkeys("bhilq", "i"), **dict.fromkeys("BHILQ", "u"), "f": "f", "d": "f", "c": "c"}.get(t._type_, "?")


def declaration(text, named):
    """'const lvdgs_args *const *views' -> ('lvdgs_args', 2): the base type and the number of indirections (an array is one)."""
    words = [w for w in re.sub(r"\[[^\]]*\]|\*", " ", text).split() if w != "const"]
    if named and len(words) > 1:
        words.pop()
    return " ".join(words), text.count("*") + ("[" in text)


def read_header(path, mirror, tmp):
    """include/lvdgs.h twice over: its text gives the names -- structs, constants, prototypes --, a probe compiled from it gives
    what only the compiler knows -- every constant's value, every struct's size, and offset, size and kind of each field that
    ``mirror`` names."""
    raw = open(path).read()
    text = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    h = SimpleNamespace(raw=raw)
    h.structs = re.findall(r"typedef\s+struct\s+\w*\s*\{[^{}]*\}\s*(lvdgs_\w+)\s*;", text)
    names = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(LVDGS_[A-Z0-9_]+)[ \t]+\S", text, flags=re.M)
    for body in re.findall(r"\benum\s*\w*\s*\{([^{}]*)\}", text):
        names += re.findall(r"\bLVDGS_[A-Z0-9_]+\b", body)
    flat = re.sub(r"\{[^{}]*\}", " ", re.sub(r"^[ \t]*#.*$", "", text, flags=re.M))      # no directives, no struct or enum bodies
    h.prototypes = {}
    for ret, name, params in re.findall(r"([\w\s\*]+?)\b(lvdgs_\w+)\s*\(([^()]*)\)\s*;", flat):
        params = [] if params.strip() == "void" else [p.strip() for p in params.split(",")]
        h.prototypes[name] = (declaration(ret, False), [(p, declaration(p, True)) for p in params])

    lines = [f'    printf("K {n} %lld\\n", (long long)({n}));' for n in dict.fromkeys(names)]
    for cname in h.structs:
        lines.append(f'    printf("S {cname} %zu\\n", sizeof({cname}));')
        cls = mirror.structs.get(cname)
        for f, t in (cls._fields_ if cls is not None else ()):
            cf = getattr(cls, "_c_field_names_", {}).get(f, f)
            kind = '"-"' if ctype_kind(t) == "-" else f"KIND((({cname} *)0)->{cf})"
            lines.append(f'    printf("F {cname} {cf} %zu %zu %s\\n", offsetof({cname}, {cf}), sizeof((({cname} *)0)->{cf}), {kind});')
    src, exe = tmp / "probe.c", tmp / "probe"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{path}"\n{KIND}\nint main(void) {{\n'
                   + "\n".join(lines) + "\n    return 0;\n}\n")
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    h.constants, h.sizes, h.fields = {}, {}, {}
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        tag, *w = line.split()
        if tag == "K":
            h.constants[w[0]] = int(w[1])
        elif tag == "S":
            h.sizes[w[0]] = int(w[1])
        else:
            h.fields[w[0], w[1]] = (int(w[2]), int(w[3]), w[4])
    return h


def accepted(base, depth, structs):
    """The ctypes types that may stand for a C parameter or return value of type ``base`` behind ``depth`` indirections."""
    if depth == 0:
        return [None] if base == "void" else [SCALARS[base]] if base in SCALARS else []
    if base in structs:      # a mirrored struct: its own pointer type, nothing looser
        t = structs[base]
        for _ in range(depth):
            t = C.POINTER(t)
        return [t]
    ok = [C.c_void_p] + [C.c_char_p] * (base == "char" and depth == 1) + [C.POINTER(C.c_void_p)] * (depth == 2)
    if base in SCALARS:
        t = SCALARS[base]
        for _ in range(depth):
            t = C.POINTER(t)
        ok.append(t)
    return ok


def mismatches(h, m):
    """Everything in which the mirror ``m`` (``mirror_of``) disagrees with the header ``h`` (``read_header``), one line each."""
    bad = [f"struct {n}: in the header, not mirrored" for n in h.structs if n not in m.structs]
    bad += [f"struct {n}: mirrored, not in the header" for n in m.structs if n not in h.structs]
    for cname, cls in m.structs.items():
        if cname not in h.sizes:
            continue
        if C.sizeof(cls) != h.sizes[cname]:
            bad.append(f"struct {cname}: sizeof {C.sizeof(cls)}, C {h.sizes[cname]}")
        for f, t in cls._fields_:
            cf = getattr(cls, "_c_field_names_", {}).get(f, f)
            mine = (getattr(cls, f).offset, C.sizeof(t), ctype_kind(t))
            if (cname, cf) not in h.fields:
                bad.append(f"field {cname}.{cf}: not probed")
            elif mine != h.fields[cname, cf]:
                bad.append(f"field {cname}.{cf}: (offset, size, kind) {mine}, C {h.fields[cname, cf]}")

    for name, value in h.constants.items():
        if name[len("LVDGS_"):] not in m.constants:
            bad.append(f"constant {name}: no mirror")
        elif m.constants[name[len("LVDGS_"):]] != value:
            bad.append(f"constant {name}: {m.constants[name[len('LVDGS_'):]]}, C {value}")
    for name, value in m.constants.items():
        if "LVDGS_" + name in h.constants:
            continue
        if name not in RESTATED:
            bad.append(f"constant {name}: neither in the header nor on the list of restated values")
        elif RESTATED[name][0] not in " ".join(h.raw.split()) or RESTATED[name][1] != value:
            bad.append(f"constant {name}: {value}, restates {RESTATED[name]}")

    bad += [f"prototype {n}: declared, not in PROTOTYPES" for n in h.prototypes if n not in m.prototypes]
    bad += [f"prototype {n}: in PROTOTYPES, not declared" for n in m.prototypes if n not in h.prototypes]
    for name, (ret, params) in h.prototypes.items():
        if name not in m.prototypes:
            continue
        restype, argtypes = m.prototypes[name]
        if restype not in accepted(*ret, m.structs):
            bad.append(f"prototype {name}: returns {restype}, C {ret}")
        if len(argtypes) != len(params):
            bad.append(f"prototype {name}: {len(argtypes)} argtypes, C {len(params)} parameters")
        for i, (t, (text, decl)) in enumerate(zip(argtypes, params)):
            if t not in accepted(*decl, m.structs):
                bad.append(f"prototype {name}: argument {i} is {t}, C '{text}'")
    return bad


@pytest.fixture(scope="module")
def mirror():
    return mirror_of(_abi)


@pytest.fixture(scope="module")
def header(mirror, tmp_path_factory):
    return read_header(HEADER, mirror, tmp_path_factory.mktemp("abi"))


def test_the_mirror_is_the_header(header, mirror):
    """Every struct (size; offset, size and kind of every field), every constant and every prototype, both ways."""
    assert header.structs and header.constants and header.prototypes
    assert set(header.fields) >= {("lvdgs_args", "tile_row_end"), ("lvdgs_map_edit_column", "in"), ("lvdgs_kernel_time", "name")}
    bad = mismatches(header, mirror)
    assert not bad, "\n".join(bad)
    assert list(mirror.prototypes) == list(header.prototypes)      # PROTOTYPES keeps the header's order
    assert all("LVDGS_" + n not in header.constants for n in RESTATED)


def test_flags_are_distinct_single_bits(header):
    flags = [v for n, v in header.constants.items() if n.startswith("LVDGS_FLAG_")]
    assert flags and len(set(flags)) == len(flags) and all(v > 0 and v & (v - 1) == 0 for v in flags)


def test_the_info_words_are_the_readable_names(header):
    words = {n: v for n, v in header.constants.items() if n.startswith("LVDGS_DYNAMIC_MASK_INFO_") and n != "LVDGS_DYNAMIC_MASK_INFO_WORDS"}
    assert sorted(words.values()) == list(range(len(_abi.DYNAMIC_MASK_INFO)))
    assert len(words) <= _abi.DYNAMIC_MASK_INFO_WORDS


def test_frame_eval_row_dtype_is_the_struct():
    row = _abi.FrameEvalRow
    assert C.sizeof(row) == _abi.FRAME_EVAL_ROW_BYTES == _abi.FRAME_EVAL_ROW_DTYPE.itemsize
    assert _abi.FRAME_EVAL_ROW_DTYPE.names == tuple(f for f, _ in row._fields_)
    for f, t in row._fields_:
        dt, offset = _abi.FRAME_EVAL_ROW_DTYPE.fields[f][:2]
        assert (offset, dt.itemsize, dt.kind) == (getattr(row, f).offset, C.sizeof(t), ctype_kind(t)), f


def variant(cls, fields):
    return type(cls.__name__, (C.Structure,), {"_c_name_": cls._c_name_, "_fields_": fields})


def test_the_checker_reports_a_wrong_mirror_by_name(header, mirror):
    def report(**changed):
        wrong = copy.copy(mirror)
        for part, (key, value) in changed.items():
            setattr(wrong, part, {**getattr(mirror, part), key: value})
        return mismatches(header, wrong)

    fields = list(_abi.LossArgs._fields_)
    swapped = [fields[1], fields[0]] + fields[2:]      # width <-> height: the same sizes, the other offsets
    bad = report(structs=("lvdgs_loss_args", variant(_abi.LossArgs, swapped)))
    assert any(b.startswith("field lvdgs_loss_args.width:") for b in bad) and any(b.startswith("field lvdgs_loss_args.height:") for b in bad)
    as_float = [(f, C.c_float if f == "weight_by_opacity" else t) for f, t in fields]      # int32_t in the header
    bad = report(structs=("lvdgs_loss_args", variant(_abi.LossArgs, as_float)))
    at = _abi.LossArgs.weight_by_opacity.offset
    assert [b for b in bad if b.startswith("field ")] == [f"field lvdgs_loss_args.weight_by_opacity: (offset, size, kind) ({at}, 4, 'f'), C ({at}, 4, 'i')"]
    assert report(constants=("FLAG_NO_BLEND", _abi.FLAG_NO_BLEND + 1)) == ["constant LVDGS_FLAG_NO_BLEND: 9, C 8"]
    assert report(prototypes=("lvdgs_binning_bytes", (C.c_size_t, [C.c_int32]))) == \
        ["prototype lvdgs_binning_bytes: argument 0 is %s, C 'int64_t num_rendered'" % C.c_int32]
    short = copy.copy(mirror)
    short.prototypes = {n: p for n, p in mirror.prototypes.items() if n != "lvdgs_profile_reset"}
    assert mismatches(header, short) == ["prototype lvdgs_profile_reset: declared, not in PROTOTYPES"]
    # what the mirror got wrong before this test existed
    assert report(prototypes=("lvdgs_profile_enable", (C.c_int, [C.c_int]))) == ["prototype lvdgs_profile_enable: returns %s, C ('void', 0)" % C.c_int]
    assert report(prototypes=("lvdgs_forward", (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p])))      # a struct's pointer, untyped
    assert report(constants=("SEED_EXTRA", 5)) == ["constant SEED_EXTRA: neither in the header nor on the list of restated values"]


def test_every_lib_attribute_the_tree_uses_exists():
    """Every attribute of _lib that a file importing this package's _lib names (``DEPTH_ALIGN_*`` in prose names none)."""
    importer = re.compile(r"^\s*(?:from\s+(?:lvdgs|\.)\s+import\s.*\b_lib\b|from\s+(?:lvdgs)?\._lib\s+import\s+(.*))", re.M)
    files = [os.path.join(ROOT, f) for f in ("bench.py", "__graft_entry__.py")]
    for top in ("lvd_gs-slam_amd", "tools", "tests", os.path.join("profiles", "experiments")):
        for dirpath, _, names in os.walk(os.path.join(ROOT, top)):
            files += [os.path.join(dirpath, n) for n in names if n.endswith(".py")]
    users, missing = 0, []
    for path in files:
        text = open(path, errors="ignore").read()
        found = importer.findall(text)
        if not found:
            continue
        users += 1
        names = set(re.findall(r"(?<![\w.])_lib\.([A-Za-z_]\w*)(?![\w*])", text))
        for imported in filter(None, found):
            names |= {part.split()[0] for part in imported.split("#")[0].strip("() ").split(",") if part.strip()}
        missing += [(os.path.relpath(path, ROOT), n) for n in sorted(names) if not hasattr(_lib, n)]
    assert users and not missing, missing


def test_abi_module_needs_neither_torch_nor_the_library():
    code = ("import sys; sys.path.insert(0, %r); import lvdgs; from lvdgs import _abi; "
            "assert 'torch' not in sys.modules and 'lvdgs._lib' not in sys.modules; print(len(_abi.PROTOTYPES))" % ROOT)
    assert int(subprocess.check_output([sys.executable, "-c", code])) == len(_lib.EXPORTS)


# ---------------------------------------------------------------- the loaded library
def test_library_loads_and_reports_version():
    L = _lib.lib()
    assert b"gfx950" in L.lvdgs_version()


def test_every_declared_symbol_is_exported():
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(lvdgs_[a-z0-9_]+)\s*\(", text))
    declared -= {"lvdgs_status"}
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name), name


def test_pose_and_adam_argument_validation_without_gpu():
    L = _lib.lib()
    pa = _lib.PoseStepArgs()
    assert L.lvdgs_pose_step(C.byref(pa), None) == _lib.E_INVALID and b"NULL" in L.lvdgs_last_error()
    arr = (_lib.AdamTensor * 8)()
    assert L.lvdgs_adam_step(arr, 9, 0.9, 0.999, 1e-15, None) == _lib.E_INVALID
    assert L.lvdgs_adam_step(arr, 1, 1.0, 0.999, 1e-15, None) == _lib.E_INVALID and b"betas" in L.lvdgs_last_error()
    arr[0].numel, arr[0].step = 4, 0
    assert L.lvdgs_adam_step(arr, 1, 0.9, 0.999, 1e-15, None) == _lib.E_INVALID      # step counts start at 1
    arr[0].step = 1
    assert L.lvdgs_adam_step(arr, 1, 0.9, 0.999, 1e-15, None) == _lib.E_INVALID and b"NULL" in L.lvdgs_last_error()
    assert L.lvdgs_adam_step(arr, 0, 0.9, 0.999, 1e-15, None) == _lib.OK             # nothing to do
    md = _lib.MaskedDepthArgs()
    assert L.lvdgs_masked_depth_l1_forward(C.byref(md), None) == _lib.E_INVALID
    ml = _lib.MaskedLossArgs()
    views = (C.POINTER(_lib.MaskedLossArgs) * 1)(C.pointer(ml))
    assert L.lvdgs_masked_loss_batch(views, 1, None) == _lib.E_INVALID and b"image size" in L.lvdgs_last_error()
    ml.width, ml.height = 64, 48
    assert L.lvdgs_masked_loss_batch(views, 1, None) == _lib.E_INVALID and b"NULL" in L.lvdgs_last_error()
    assert L.lvdgs_masked_loss_batch(views, 0, None) == _lib.OK
    assert L.lvdgs_masked_loss_scratch_bytes(1226, 370) % 256 == 0 and L.lvdgs_masked_loss_scratch_bytes(1226, 370) >= 4 * 39 * 12 * 8
    a = _lib.Args()
    assert L.lvdgs_backward_masked_loss(C.byref(a), C.byref(ml), None) == _lib.E_INVALID
    assert L.lvdgs_blend_backward_window_batch(None, None, None, 1, 0, None) == _lib.E_INVALID


def test_sizes_are_monotone_and_aligned():
    L = _lib.lib()
    assert L.lvdgs_geom_bytes(0) > 0
    prev = 0
    for n in (1, 1000, 100_000, 2_000_000):
        b = L.lvdgs_geom_bytes(n)
        assert b % 256 == 0 and b > prev and b >= n * 60
        prev = b
    assert L.lvdgs_binning_bytes(3_000_000) >= 3_000_000 * 8
    assert L.lvdgs_image_bytes(1920, 1080) >= 1920 * 1080 * 8
    assert L.lvdgs_backward_scratch_bytes(500_000, 3_000_000) >= 3_000_000 * 40   # ten floats per (Gaussian, tile) pair


def test_argument_validation_without_gpu():
    L = _lib.lib()
    a = _lib.Args()
    n = C.c_int64(-1)
    assert L.lvdgs_forward_prepare(C.byref(a), C.byref(n), None) == _lib.E_INVALID
    assert b"image size" in L.lvdgs_last_error()
    a.image_width, a.image_height, a.tanfovx, a.tanfovy = 64, 64, 1.0, 1.0
    assert L.lvdgs_forward_prepare(C.byref(a), C.byref(n), None) == _lib.E_INVALID  # bg / matrices NULL
    a.sh_degree = 7
    assert L.lvdgs_forward_render(C.byref(a), None) == _lib.E_INVALID
    assert b"sh_degree" in L.lvdgs_last_error()
    with pytest.raises(_lib.LvdgsError):
        _lib.check(_lib.E_INVALID, "probe")


def test_every_export_is_in_the_integration_guide():
    """INTEGRATION.md's binding table names every entry point include/lvdgs.h declares (what each replaces on the reference's side)."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    missing = [n for n in _lib.EXPORTS if n not in doc]
    assert not missing, missing


def test_gaussian_backward_batch_argument_validation_without_gpu():
    """lvdgs_gaussian_backward_batch refuses view lists it has no single launch for -- before anything is enqueued."""
    L = _lib.lib()
    assert L.lvdgs_gaussian_backward_batch(None, 0, None) == _lib.OK   # nothing to do
    assert L.lvdgs_gaussian_backward_batch(None, 2, None) == _lib.E_INVALID and b"view list" in L.lvdgs_last_error()
    a, b = _lib.Args(), _lib.Args()
    views = (C.POINTER(_lib.Args) * 2)(C.pointer(a), C.pointer(b))
    a.flags = b.flags = _lib.FLAG_POSE_ONLY
    assert L.lvdgs_gaussian_backward_batch(views, 2, None) == _lib.E_INVALID and b"POSE_ONLY" in L.lvdgs_last_error()
    a.flags = b.flags = 0
    assert L.lvdgs_gaussian_backward_batch(views, 2, None) == _lib.E_INVALID and b"one coefficient" in L.lvdgs_last_error()   # no shs
    a.shs = b.shs = 256   # (never dereferenced: every call here is rejected before a launch)
    a.sh_coeffs = b.sh_coeffs = 1
    b.num_gaussians = 5
    assert L.lvdgs_gaussian_backward_batch(views, 2, None) == _lib.E_INVALID and b"differ in map" in L.lvdgs_last_error()
    b.num_gaussians = 0
    assert L.lvdgs_gaussian_backward_batch(views, 2, None) == _lib.E_INVALID and b"ACCUMULATE_PARAM_GRADS" in L.lvdgs_last_error()
    views[1] = None
    assert L.lvdgs_gaussian_backward_batch(views, 2, None) == _lib.E_INVALID and b"view 1 is NULL" in L.lvdgs_last_error()


def test_rope2d_strided_argument_validation_without_gpu():
    L = _lib.lib()
    tok, pos = C.c_void_p(256), C.c_void_p(512)  # never dereferenced: every call below is rejected before a launch
    call = lambda dtype, B, N, H, D, sb, sn, sh: L.lvdgs_rope2d_strided(tok, dtype, pos, B, N, H, D, sb, sn, sh, 100.0, 1.0, None)
    assert call(0, 1, 4, 2, 6, 48, 12, 6) == _lib.E_INVALID and b"multiple of 4" in L.lvdgs_last_error()
    assert call(3, 1, 4, 2, 8, 64, 16, 8) == _lib.E_INVALID and b"dtype" in L.lvdgs_last_error()
    assert call(1, 1, 4, 2, 8, 64, 16, 4) == _lib.E_INVALID and b"strides" in L.lvdgs_last_error()   # heads overlap
    assert call(2, 1, 4, 2, 8, 64, -16, 8) == _lib.E_INVALID
    assert call(0, 0, 4, 2, 8, 64, 16, 8) == _lib.OK                                                    # no tokens: nothing to do
    assert L.lvdgs_rope2d_strided(None, 0, pos, 1, 4, 2, 8, 64, 16, 8, 100.0, 1.0, None) == _lib.E_INVALID


def test_product_package_never_imports_the_oracle():
    """The product path may not import, link or execute anything under oracle/."""
    pkg = os.path.join(ROOT, "lvd_gs-slam_amd")
    bad = re.compile(r"import\s+oracle|from\s+oracle|oracle/|oracle\.py|liblvdgs_oracle|lvdgs_oracle")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp")) or f == "Makefile":
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert not bad.search(text), (dirpath, f)


def test_rasterizer_refuses_cpu_tensors():
    import torch
    from lvdgs.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    rs = GaussianRasterizationSettings(16, 16, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), torch.eye(4),
                                       0, torch.zeros(3))
    with pytest.raises(_lib.LvdgsError):
        GaussianRasterizer(rs)(means3D=torch.zeros(2, 3), means2D=torch.zeros(2, 3), opacities=torch.ones(2, 1),
                               colors_precomp=torch.ones(2, 3), scales=torch.ones(2, 3), rotations=torch.ones(2, 4))
