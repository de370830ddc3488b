"""CPU: the ctypes binding that hover_net_amd/lib.py generates from include/hvn.h -- the header is the only description of the ABI.
Struct layouts are held to a compiler's `sizeof` / `offsetof`, the export list to the built library's dynamic symbols, and every
prototype to the argtypes / restype that `lib()` sets; the table below pins the facts the per-feature tests used to pin."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from hover_net_amd import augment, features, lib as L, patching, post_proc

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc (host-only use: no GPU, no HIP runtime)")

ARG_COUNTS = {"hvn_viz_strip": 18, "hvn_augment_shape_images": 18, "hvn_tissue_gray_hist": 6, "hvn_tissue_mask_workspace_bytes": 2,
              "hvn_tissue_mask": 13, "hvn_valid_stats": 14}
SIZES = {"hvn_view": 48, "hvn_op": 392, "hvn_top": 336, "hvn_pack_desc": 48, "hvn_loss": 152, "hvn_inst_rec": 48, "hvn_inst_feat": 88,
         "hvn_aug_sample": 128, "hvn_image_rec": 16, "hvn_patch_rec": 12}
DTYPES = {"hvn_inst_rec": post_proc._REC_DTYPE, "hvn_inst_feat": features.FEAT_DTYPE, "hvn_aug_sample": augment.AUG_DTYPE,
          "hvn_image_rec": patching.IMAGE_DTYPE, "hvn_patch_rec": patching.PATCH_DTYPE}
AUG_NAMES = ("inv", "src", "flip_lr", "flip_ud", "kind", "p0", "p1", "per_channel", "noise_scale", "order", "hue", "sat", "bright", "contrast")
FEATURE_SOURCES = ("hvn_resample.hip", "hvn_features.hip", "hvn_tissue.hip", "hvn_viz.hip", "hvn_valid.hip", "hvn_augment.hip")


def test_pinned_facts():
    lib = L.lib()
    assert lib.hvn_version() == 104
    assert len(L.EXPORTS) == len(set(L.EXPORTS)) == 53 and set(L.EXPORTS) == set(L.PROTOS)
    for name in L.EXPORTS:
        assert hasattr(lib, name), name
    for name, n in ARG_COUNTS.items():
        assert len(getattr(lib, name).argtypes) == n, name
    assert lib.hvn_tissue_mask_workspace_bytes.restype is ctypes.c_size_t
    assert list(L.STRUCTS) == ["hvn_view", "hvn_op", "hvn_inst_rec", "hvn_inst_feat", "hvn_pack_desc", "hvn_top", "hvn_loss",
                               "hvn_aug_sample", "hvn_image_rec", "hvn_patch_rec"]
    for name, size in SIZES.items():
        assert ctypes.sizeof(getattr(L, name)) == size, name
    for name, dt in DTYPES.items():
        assert dt.itemsize == SIZES[name] and dt.names == tuple(f[0] for f in getattr(L, name)._fields_), name
    assert features.FEAT_DTYPE.itemsize == ctypes.sizeof(L.hvn_inst_feat) == 88
    assert augment.AUG_DTYPE.itemsize == 128 and augment.AUG_DTYPE.fields["order"][1] == 80 and augment.AUG_DTYPE.fields["hue"][1] == 96
    assert augment.AUG_DTYPE.names == AUG_NAMES
    assert patching.IMAGE_DTYPE.itemsize == 16 and patching.PATCH_DTYPE.itemsize == 12
    assert L.hvn_top._fields_[[f[0] for f in L.hvn_top._fields_].index("net")][1] is ctypes.POINTER(L.hvn_op)
    for src in FEATURE_SOURCES:
        assert src in L.SOURCES and os.path.isfile(os.path.join(L.CSRC, src)), src


def test_every_prototype_is_bound():
    """After lib(), every function of the header has the prototype's argtypes and restype; the type of each parameter is read here a
    second time, from the declaration's text, by the rule "a pointer or an array is a void*, a scalar is its own ctypes type"."""
    lib = L.lib()
    text = re.sub(r"/\*.*?\*/", " ", open(L.HEADER).read(), flags=re.S)
    scalar = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "long": ctypes.c_long,
              "float": ctypes.c_float, "double": ctypes.c_double}
    decls = re.findall(r"HVN_API\s+([\w\s]+?\*?)\s*(hvn_\w+)\s*\(([^)]*)\)\s*;", text)
    assert [d[1] for d in decls] == list(L.EXPORTS)
    for ret, name, args in decls:
        fn = getattr(lib, name)
        params = [] if args.strip() == "void" else [a.strip() for a in args.split(",")]
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), name
        for got, p in zip(fn.argtypes, params):
            want = ctypes.c_void_p if ("*" in p or "[" in p) else scalar[p.replace("const ", "").rsplit(None, 1)[0]]
            assert got is want, (name, p)
        assert fn.restype is (ctypes.c_char_p if "*" in ret else scalar[ret.strip()]), name


def _flat(struct, prefix=""):
    """(dotted C member path, offset, size) of every field of a ctypes struct, nested structs followed."""
    for name, t in struct._fields_:
        f = getattr(struct, name)
        yield prefix + name, f.offset, f.size
        if isinstance(t, type) and issubclass(t, ctypes.Structure):
            for sub, off, size in _flat(t, prefix + name + "."):
                yield sub, f.offset + off, size


@needs_hipcc
def test_layouts_against_the_compiler(tmp_path):
    """sizeof and every offsetof as the build's own driver sees them in a plain host C program, against the generated ctypes classes
    and the numpy dtypes made of them."""
    lines = ['#include <stdio.h>', '#include "hvn.h"', 'int main(void) {']
    for sname, struct in L.STRUCTS.items():
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (sname, sname))
        for path, _off, _size in _flat(struct):
            lines.append('    printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (sname, path, sname, path, sname, path))
    lines += ['    return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["hipcc", "-x", "c", "-I", os.path.dirname(L.HEADER), str(src), "-o", str(exe)], check=True, timeout=300)
    out = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, timeout=60).stdout.decode().split("\n")
    seen = {ln.split()[0]: tuple(int(v) for v in ln.split()[1:]) for ln in out if ln.strip()}
    want = {}
    for sname, struct in L.STRUCTS.items():
        want[sname] = (ctypes.sizeof(struct),)
        for path, off, size in _flat(struct):
            want["%s.%s" % (sname, path)] = (off, size)
    assert seen == want, {k: (seen.get(k), want.get(k)) for k in set(seen) | set(want) if seen.get(k) != want.get(k)}
    for sname, dt in DTYPES.items():
        assert dt == np.dtype(L.STRUCTS[sname]), sname
        assert dt.itemsize == seen[sname][0], sname
        for name in dt.names:
            sub, off = dt.fields[name][:2]
            assert (off, sub.itemsize) == seen["%s.%s" % (sname, name)], (sname, name)


@needs_hipcc
def test_exports_both_ways():
    """The dynamic hvn_* symbols the built library defines are exactly the functions the header declares (the dynamic symbol table
    as the llvm-objdump next to the build's compiler prints it: `llvm-nm -D --defined-only` where ROCm ships llvm-nm)."""
    version = subprocess.run(["hipcc", "--version"], check=True, stdout=subprocess.PIPE, timeout=60).stdout.decode()
    objdump = os.path.join(re.search(r"InstalledDir:\s*(\S+)", version).group(1), "llvm-objdump")
    out = subprocess.run([objdump, "-T", L.lib_path()], check=True, stdout=subprocess.PIPE, timeout=60).stdout.decode()
    defined = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("hvn_") and "*UND*" not in ln}
    assert "hvn_version" in defined
    assert defined == set(L.EXPORTS), defined ^ set(L.EXPORTS)


HEADER_OK = """
typedef struct hvn_a { void *base; int64_t sn, sy; int32_t h[3]; } hvn_a;
typedef struct hvn_b { hvn_a x; const hvn_a *net; const float *w, *bias; double d; } hvn_b;
HVN_API int hvn_f(const hvn_b *ops, int n, const uint8_t rgb[3], long long out[10], size_t bytes, void *stream);
HVN_API const char *hvn_g(void);
"""


def test_parser_reads_the_forms_and_refuses_the_rest():
    structs, protos = L.parse_header(HEADER_OK)
    a, b = structs["hvn_a"], structs["hvn_b"]
    assert [(n, t) for n, t in a._fields_] == [("base", ctypes.c_void_p), ("sn", ctypes.c_int64), ("sy", ctypes.c_int64), ("h", ctypes.c_int32 * 3)]
    assert [(n, t) for n, t in b._fields_] == [("x", a), ("net", ctypes.POINTER(a)), ("w", ctypes.c_void_p), ("bias", ctypes.c_void_p),
                                               ("d", ctypes.c_double)]
    assert protos == {"hvn_f": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
                      "hvn_g": (ctypes.c_char_p, [])}
    bad = {"hvn_a": HEADER_OK.replace("int32_t h[3];", "uint16_t h[3];"),                 # a field type outside the table
           "hvn_f": HEADER_OK.replace("int n,", "unsigned n,"),                            # a parameter type outside the table
           "hvn_g": HEADER_OK.replace("const char *hvn_g", "hvn_b hvn_g"),                 # a return type outside the table
           "hvn_b": HEADER_OK.replace("double d; }", "struct { int q; } d; }"),           # a nested body: not a form of this header
           "hvn_h": HEADER_OK + "HVN_API int hvn_h(int (*cb)(int), void *stream);\n"}      # a function pointer: not a form either
    for name, text in bad.items():
        with pytest.raises(L.HvnError, match=name):
            L.parse_header(text)
