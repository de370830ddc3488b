"""ctypes binding of libhvn_hip.so, generated from include/hvn.h at import: the header is the only description of the ABI.
`parse_header` turns its structs into ctypes.Structure classes (module attributes under their header names) and its prototypes into
the argtypes / restype that `lib()` sets on every export; nothing here restates a declaration, and one the reader cannot map raises.
`stream_ptr`, `grown` and `call` are the one call path of the package's launch sites.  No fallback: if the library is missing or no
gfx950 device is visible, every entry point raises."""
import ctypes
import os
import re
import subprocess

from .knobs import knob

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libhvn_hip.so")
# Experiment builds of the same sources (`build_variant`), loaded INSTEAD of the default library when HVN_LIB_VARIANT names one:
# kernel A/B runs on one box without rebuilding there.  Not used by the product path (unset = libhvn_hip.so).
VARIANTS = {
    "fullepi": ("-DHVN_X3G_FULL_EPI=1",),           # hvn_conv_igemm_x3g with the one full epilogue of rounds 1-5: the reference tools/epilogue_forms_check.py holds the 8 operand-set forms to
    "prev": (),                                      # same-box A/B against ANOTHER CHECKOUT's library: built by hand into libhvn_hip_prev.so (never by build_variant)
    "trace": ("-DHVN_TRACE_FINE=1",),               # diagnosis: per-phase timestamps of the conv epilogue (with HVN_CONV_TRACE, tools/conv_trace.py --fine)
}
CSRC = os.path.join(_HERE, "csrc")
HEADERS = ("hvn_conv_common.h", "hvn_env.h", "hvn_error.h", "hvn_kernels.h")
SOURCES = ("hvn_conv.hip", "hvn_conv_chain.hip", "hvn_conv_chain_x3.hip", "hvn_conv_chain_x3r.hip", "hvn_conv_bf16.hip", "hvn_conv_bf16g.hip", "hvn_conv_chain_bf16.hip", "hvn_conv_x3.hip", "hvn_conv_x3g.hip", "hvn_net_ops.hip", "hvn_postproc.hip", "hvn_api.hip", "hvn_train.hip", "hvn_wgrad_x3.hip", "hvn_targets.hip", "hvn_wsi_merge.hip",
           "hvn_augment.hip", "hvn_train_api.hip", "hvn_contour.cpp", "hvn_contour_dev.hip", "hvn_metrics.hip", "hvn_valid.hip", "hvn_overlay.hip", "hvn_resample.hip", "hvn_tissue.hip", "hvn_viz.hip", "hvn_features.hip", "hvn_tta.hip", "hvn_stain.hip", "hvn_neighbours.hip", "hvn_clusters.hip", "hvn_density.hip", "hvn_pairs.hip", "hvn_pairs_sim.hip", "hvn_regions.hip", "hvn_margins.hip", "hvn_graph.hip", "hvn_forest.hip", "hvn_texture.hip")
HIPCC_FLAGS = ("--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
               "-fvisibility=hidden", "-Wno-unused-value", "-pthread")


class HvnError(RuntimeError):
    pass


HEADER = os.path.join(os.path.dirname(_HERE), "include", "hvn.h")
_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "long": ctypes.c_long,
            "float": ctypes.c_float, "double": ctypes.c_double}


def parse_header(text):
    """(structs, protos) of a header written in hvn.h's forms: every `typedef struct NAME { ... } NAME;` as a ctypes.Structure, in
    header order, and every `HVN_API <ret> name(args);` as name -> (restype, argtypes).  Not a C grammar: a declaration outside these
    forms, or of a type the tables below do not map, raises HvnError naming it -- none is ever skipped."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*|^[ \t]*#[^\n]*", " ", text, flags=re.S | re.M)
    structs, protos = {}, {}
    for chunk in re.split(r"\btypedef\s+struct\b", text)[1:]:
        m = re.match(r"\s*(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", chunk)
        if not m or m.group(1) != m.group(3):
            raise HvnError("hvn.h: cannot read `typedef struct %s ...`" % " ".join(chunk.split())[:60])
        name, body, fields = m.group(1), m.group(2), []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            base, _, rest = re.sub(r"\bconst\b", " ", decl).strip().partition(" ")
            for d in rest.split(","):
                m = re.fullmatch(r"\s*(\*?)\s*(\w+)\s*(?:\[(\d+)\])?\s*", d)
                if m and m.group(1):            # a pointer: to a struct declared above, else opaque
                    t = ctypes.POINTER(structs[base]) if base in structs else ctypes.c_void_p
                else:
                    t = structs.get(base) or _SCALARS.get(base)
                if not m or t is None:
                    raise HvnError("hvn.h: cannot map `%s` of struct %s" % (decl, name))
                fields.append((m.group(2), t * int(m.group(3)) if m.group(3) else t))
        structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields})
    for decl in re.findall(r"\bHVN_API\b([^;]*);", text):
        m = re.fullmatch(r"([^()]*?)(\w+)\s*\(([^()]*)\)\s*", decl)
        if not m:
            raise HvnError("hvn.h: cannot read `HVN_API %s`" % " ".join(decl.split()))
        ret, name, args = " ".join(m.group(1).split()), m.group(2), m.group(3)
        restype = ctypes.c_char_p if ret == "const char *" else _SCALARS.get(ret)
        params = [ctypes.c_void_p if "*" in a or "[" in a else _SCALARS.get(" ".join(a.replace("const ", " ").split()[:-1]))
                  for a in ([] if args.strip() == "void" else args.split(","))]
        if restype is None or None in params:
            raise HvnError("hvn.h: cannot map `%s %s(%s)`" % (ret, name, " ".join(args.split())))
        protos[name] = (restype, params)
    return structs, protos


# include/hvn.h is the one description of the ABI: the structs become module attributes under their header names (hvn_op, hvn_view,
# hvn_top, ...; np.dtype(<struct>) is the numpy view of a record), the prototypes the argtypes / restype that lib() sets.
STRUCTS, PROTOS = parse_header(open(HEADER).read())
globals().update(STRUCTS)
EXPORTS = tuple(PROTOS)


def source_id():
    """16 hex digits over every source the library is built from (kernels, headers, flags).  Compiled into the library
    (`hvn_build_id()`), so that a binary which does not match the sources next to it is detected at LOAD time -- the `.so` files are
    git-ignored yet travel to the GPU box, and a stale one would otherwise pass for the current kernels."""
    import hashlib

    h = hashlib.sha256()
    for f in sorted(SOURCES) + list(HEADERS):
        h.update(f.encode())
        h.update(open(os.path.join(CSRC, f), "rb").read())
    h.update(open(os.path.join(os.path.dirname(_HERE), "include", "hvn.h"), "rb").read())
    h.update(" ".join(HIPCC_FLAGS).encode())
    return h.hexdigest()[:16]


def _built_id(path):
    """The id compiled into an existing library (read from the file's bytes: dlopen would pin the old mapping in this process)."""
    if not os.path.exists(path):
        return None
    data = open(path, "rb").read()
    i = data.find(b"hvn-build-id:")
    if i < 0:
        return None
    j = data.find(b"\0", i)
    return data[i + 13:j].decode(errors="replace")


_HIPCC_VERSION = None


def _hipcc_version():
    """`hipcc --version` (bytes): part of every cached object's key -- an object built by another ROCm must not be linked."""
    global _HIPCC_VERSION
    if _HIPCC_VERSION is None:
        try:
            _HIPCC_VERSION = subprocess.run(["hipcc", "--version"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=60).stdout
        except (OSError, subprocess.SubprocessError):
            _HIPCC_VERSION = b"hipcc-unknown"
    return _HIPCC_VERSION


def _compile(out, extra, verbose):
    """One object per source, compiled in parallel and cached by the hash of what it is built from (the source, the headers, the
    flags) under csrc/.obj/, then linked: editing one kernel file recompiles that file only (~30 s instead of ~150 s for all).
    The .so still carries the id of ALL sources (`hvn_build_id`, stamped into hvn_api.hip's object)."""
    import hashlib
    from concurrent.futures import ThreadPoolExecutor

    sid = source_id() + ("" if not extra else "+" + "".join(extra))
    objdir = os.path.join(CSRC, ".obj")
    os.makedirs(objdir, exist_ok=True)
    hdr = b"".join(open(os.path.join(CSRC, f), "rb").read() for f in HEADERS) + open(os.path.join(os.path.dirname(_HERE), "include", "hvn.h"), "rb").read()
    cflags = [f for f in HIPCC_FLAGS if f != "-shared"] + list(extra)
    jobs, objs = [], []
    for src in SOURCES:
        defs = ['-DHVN_BUILD_ID="%s"' % sid] if src == "hvn_api.hip" else []
        h = hashlib.sha256(open(os.path.join(CSRC, src), "rb").read() + hdr + " ".join(cflags + defs).encode() + _hipcc_version()).hexdigest()[:16]
        obj = os.path.join(objdir, "%s.%s.o" % (src, h))
        objs.append(obj)
        if not os.path.exists(obj):
            tag = os.path.join(objdir, "%s.flags-%s" % (src, hashlib.sha256(" ".join(extra).encode()).hexdigest()[:8]))
            if os.path.exists(tag):                 # one cached object per (source, flag set): drop the one this flag set built before
                old = open(tag).read().strip()
                if old and os.path.exists(os.path.join(objdir, old)):
                    os.remove(os.path.join(objdir, old))
            open(tag, "w").write(os.path.basename(obj))
            jobs.append(["hipcc", *cflags, *defs, "-c", os.path.join(CSRC, src), "-o", obj])

    def run(cmd):
        # hipcc writes its output in place: compile / link to a private name and rename on success, so that a build killed mid-write
        # (the GPU scripts wrap everything in `timeout`) or two ranks building at once never leave a truncated file under the final name
        if verbose:
            print(" ".join(cmd))
        final = cmd[-1]
        tmp = "%s.tmp.%d" % (final, os.getpid())
        try:
            subprocess.check_call(cmd[:-1] + [tmp])
            os.replace(tmp, final)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)

    with ThreadPoolExecutor(max_workers=min(8, max(1, len(jobs)))) as ex:
        list(ex.map(run, jobs))
    run(["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread", *objs, "-o", out])
    return out


def build(verbose=False):
    """hipcc cross-compiles for gfx950 without a GPU (under a minute).  Rebuilds whenever the id compiled into the existing
    library differs from the id of the sources (not by mtime)."""
    if _built_id(LIB_PATH) == source_id():
        return LIB_PATH
    return _compile(LIB_PATH, (), verbose)


def build_variant(name, verbose=False):
    """`libhvn_hip_<name>.so`: the library compiled with VARIANTS[name]'s extra flags."""
    out = os.path.join(_HERE, "libhvn_hip_%s.so" % name)
    if _built_id(out) == source_id() + "+" + "".join(VARIANTS[name]):
        return out
    return _compile(out, tuple(VARIANTS[name]), verbose)


def lib_path():
    v = knob("HVN_LIB_VARIANT")
    if not v:
        return LIB_PATH
    if v not in VARIANTS:
        raise HvnError("HVN_LIB_VARIANT=%r: unknown variant (known: %s)" % (v, ", ".join(VARIANTS)))
    return os.path.join(_HERE, "libhvn_hip_%s.so" % v)


_LIB = None


def lib():
    """The loaded library (ctypes.CDLL); raises HvnError if it has not been built."""
    global _LIB
    if _LIB is None:
        path = lib_path()
        if not os.path.exists(path):
            raise HvnError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback for the HoVer-Net hot path)" % os.path.basename(path))
        # torch ships its own libamdhip64 and must load it FIRST: a process that dlopens this library before importing torch ends up
        # with the system HIP runtime for these kernels and torch's for the streams / allocations handed to them (hvn_device_ok then
        # fails on a GPU box: `build(); smoke()` in one process did, round 4).  Loading torch here makes the order deterministic.
        import torch  # noqa: F401
        L = ctypes.CDLL(path)
        L.hvn_build_id.restype = ctypes.c_char_p
        built = L.hvn_build_id().decode()
        if os.path.isdir(CSRC) and not knob("HVN_LIB_VARIANT") and built != source_id():
            raise HvnError("%s was built from other sources (library %s, sources %s): run `python -c 'import __graft_entry__ as g; g.build()'`"
                           % (os.path.basename(path), built, source_id()))
        for name, (restype, argtypes) in PROTOS.items():
            fn = getattr(L, name, None)
            if fn is None:
                if knob("HVN_LIB_VARIANT"):   # another checkout's library (variant "prev") may predate an entry point
                    continue
                raise HvnError("%s does not export %s, which include/hvn.h declares" % (os.path.basename(path), name))
            fn.restype, fn.argtypes = restype, argtypes
        _LIB = L
    return _LIB


def stream_ptr(device=None, stream=None):
    """hipStream_t of `stream`, or of `device`'s current stream, as the void* every entry point takes."""
    if stream is None:
        import torch
        stream = torch.cuda.current_stream(device)
    return ctypes.c_void_p(stream.cuda_stream)


def grown(buf, nbytes, device):
    """`buf` if it already holds `nbytes`, else a fresh uint8 workspace of that size (the caller keeps whichever cache it had)."""
    if buf is not None and buf.numel() >= nbytes:
        return buf
    import torch
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def call(name, *args):
    """One status-returning entry point: raises HvnError with the library's text unless it returns HVN_OK."""
    check(getattr(lib(), name)(*args), name)


def check(rc, what):
    if rc != 0:
        raise HvnError("%s failed (%d): %s" % (what, rc, lib().hvn_last_error().decode()))


def require_gpu():
    if not lib().hvn_device_ok():
        raise HvnError("no gfx950 (MI355X) device is current; the HoVer-Net hot path has no CPU fallback")
