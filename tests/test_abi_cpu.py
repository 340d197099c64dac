"""CPU: the ctypes binding `blvm/_hip.py` generates from include/blvm_hip.h — coverage of the header, entries pinned literally, what
the parser accepts and refuses, the struct layouts against the compiler's, the constants, and the struct packer `fill`."""
import ctypes
import os
import re
import shutil
import subprocess
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_longlong, c_size_t, c_void_p

import pytest

from blvm import _hip, ops

from conftest import ROOT

STRUCT_NAMES = ["BlvmVrnnWeights", "BlvmVrnnGrads", "BlvmVrnnDecodeWeights", "BlvmSrnnWeights", "BlvmSrnnGrads",
                "BlvmSrnnDecodeWeights", "BlvmLstmDecodeWeights", "BlvmRssmWeights", "BlvmRssmGrads"]  # fmt: skip


def test_every_declared_entry_point_is_bound_with_its_parameter_count():
    """Counted here with a regular expression of the test's own: every `blvm_*(` of the header is bound by `load()`, with as many
    argument types as the prototype has parameters."""
    header = open(os.path.join(ROOT, "include", "blvm_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    protos = dict(re.findall(r"\b(blvm_\w+)\s*\(([^()]*)\)\s*;", code))
    assert len(protos) >= 111 and set(protos) == set(re.findall(r"\b(blvm_\w+)\s*\(", code)) == set(_hip.SIGNATURES)
    lib = _hip.load()
    for name, params in protos.items():
        n = 0 if params.strip() in ("", "void") else params.count(",") + 1
        fn = getattr(lib, name)
        assert len(fn.argtypes) == n, name
        assert (fn.restype, list(fn.argtypes)) == _hip.SIGNATURES[name], name
    assert sorted(_hip.STRUCTS) == sorted(STRUCT_NAMES) == sorted(re.findall(r"typedef\s+struct\s+(\w+)", code))


def test_one_entry_point_per_kind_of_type_is_pinned_literally():
    """Independent of the header's text: the full (restype, argtypes) of one entry point per kind of C type the parser maps."""
    vw = POINTER(_hip.VrnnWeights)
    pinned = {
        "blvm_elbo_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_double, c_double, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
        "blvm_mix_sample": (c_int, [c_void_p] * 3 + [c_longlong] + [c_int] * 2 + [c_float] * 3 + [c_void_p] * 2),
        "blvm_gemm_ws_route": (c_int, [c_int, c_int, c_int, c_int, c_size_t, c_int, c_int, c_int, c_int, c_int]),
        "blvm_act_bwd_f32": (c_int, [c_void_p, c_void_p, c_float, c_void_p, c_size_t, c_void_p]),
        "blvm_dmol_bwd_fused_workspace_floats": (c_size_t, [c_int] * 3),
        "blvm_last_error": (c_char_p, []),
        "blvm_rnn_path_counts": (c_int, [c_void_p]),
        "blvm_gemm_arm": (c_int, [c_int] * 5 + [c_size_t, c_int, c_size_t] + [c_int] * 8),
        "blvm_wgrad_group_route": (c_int, [c_int, c_void_p, c_void_p, c_int] + [c_void_p] * 5 + [c_int, c_void_p]),
        "blvm_gemm_arm_counts": (c_int, [c_void_p]),
        "blvm_async_errors_take": (c_int, [c_void_p]),
        "blvm_wgrad_group_f32": (c_int, [c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p]),
        "blvm_vrnn_seq_bwd": (c_int, [vw, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float, c_int, c_int, c_int, c_int, c_int, c_int,
                                      c_int, c_float, c_void_p, c_void_p, POINTER(_hip.VrnnGrads), c_void_p, c_void_p]),
        "blvm_gru_seq_bwd": (c_int, [c_void_p] * 3 + [c_int, c_void_p, c_int, c_void_p, c_void_p, c_longlong, c_int] + [c_int] * 4
                             + [c_void_p, c_int, c_int] + [c_void_p] * 7),
    }  # fmt: skip
    for name, sig in pinned.items():
        assert _hip.SIGNATURES[name] == sig, name


SYNTHETIC = """
/* a comment that names blvm_not_a_function(int) and typedef struct Nothing */
#ifndef X_H
#define X_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
#define BLVM_ZERO 0
#define BLVM_MINUS (-7) /* parenthesised */
#define BLVM_PLAIN_MINUS -3
typedef struct BlvmInner {
  const float *a[2], *b; /* several declarators on a line */
  float *c;
} BlvmInner;
typedef struct BlvmOuter { const BlvmInner* inner; const float *const *rows; float *d[4]; } BlvmOuter;
int blvm_nothing(void);
const char* blvm_text(void);
size_t blvm_count(int a, unsigned b, float c, double d, size_t e, long long f, int32_t g, const int h);
int blvm_pointers(const BlvmOuter* w, BlvmInner* g, const float* x, float* y, const int32_t* lens, unsigned* code,
                  unsigned long long out[12], unsigned long long* buf, const float* const* D, float* const* dW, size_t* n,
                  double* acc, void* stream);  // spans lines
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_accepts_every_form_the_header_uses():
    structs, sigs, constants = _hip.parse_header(SYNTHETIC)
    assert constants == {"BLVM_ZERO": 0, "BLVM_MINUS": -7, "BLVM_PLAIN_MINUS": -3}
    inner, outer = structs["BlvmInner"], structs["BlvmOuter"]
    assert list(structs) == ["BlvmInner", "BlvmOuter"]
    assert inner._fields_ == [("a", c_void_p * 2), ("b", c_void_p), ("c", c_void_p)]
    assert outer._fields_ == [("inner", POINTER(inner)), ("rows", POINTER(c_void_p)), ("d", c_void_p * 4)]
    assert sigs == {
        "blvm_nothing": (c_int, []),
        "blvm_text": (c_char_p, []),
        "blvm_count": (c_size_t, [c_int, ctypes.c_uint, c_float, c_double, c_size_t, c_longlong, ctypes.c_int32, c_int]),
        "blvm_pointers": (c_int, [POINTER(outer), POINTER(inner)] + [c_void_p] * 11),
    }


@pytest.mark.parametrize(
    "declaration",
    [
        "int blvm_x(short n);",
        "typedef struct BlvmVrnnWeights { const float *a; } BlvmVrnnWeights;\nint blvm_x(BlvmVrnnWeights w);",
        "int blvm_x(void (*cb)(int), void* stream);",
        "int blvm_x(const char* fmt, ...);",
        "int blvm_y(int a);\nint blvm_x(int a)",
        "int blvm_x(int a)\nint blvm_y(int a);",
        "void blvm_x(int a);",
        "int blvm_x(struct Foo* p);",
        "int blvm_x(Foo* p);",
        "typedef struct BlvmS { int n; } BlvmS;",
        "typedef struct BlvmS { const float *a; struct { float *b; } in; } BlvmS;",
    ],
)
def test_parser_refuses_what_lies_outside_the_subset(declaration):
    """A type outside the list, a struct by value, a function pointer, an ellipsis, a prototype without its `;` (last in the file and
    in front of another), another return type, a pointer to an unknown type, a member that is no pointer, a nested struct: each raises
    and quotes the declaration with `blvm_x` (or the struct) in it."""
    quoted = "BlvmS" if "BlvmS" in declaration else "blvm_x"
    with pytest.raises(_hip.BlvmHipError, match=quoted):
        _hip.parse_header("#define BLVM_OK 0\n" + declaration + "\n")


def test_grads_structs_are_the_twins_of_their_weights():
    for kind in ("Vrnn", "Srnn", "Rssm"):
        w, g = _hip.STRUCTS[f"Blvm{kind}Weights"], _hip.STRUCTS[f"Blvm{kind}Grads"]
        assert w is not g and g._fields_ == w._fields_ and len(w._fields_) >= 8, kind
    assert (_hip.VrnnGrads, _hip.SrnnGrads, _hip.RssmGrads) == tuple(_hip.STRUCTS[f"Blvm{k}Grads"] for k in ("Vrnn", "Srnn", "Rssm"))
    for name in ("VrnnWeights", "VrnnDecodeWeights", "SrnnWeights", "SrnnDecodeWeights", "LstmDecodeWeights", "RssmWeights"):
        assert getattr(_hip, name) is _hip.STRUCTS["Blvm" + name]


def test_constants_come_from_the_header():
    want = {"BLVM_OK": 0, "BLVM_EINVAL": -1, "BLVM_ELAUNCH": -2, "BLVM_ENOSUP": -3, "BLVM_NOT_APPLICABLE": 1,
            "BLVM_DTYPE_F32": 0, "BLVM_DTYPE_BF16": 1, "BLVM_DTYPE_F16": 2}  # fmt: skip
    assert {name: _hip.CONSTANTS.get(name) for name in want} == want
    assert ops.BLVM_NOT_APPLICABLE == 1 and _hip.DTYPES == {"f32": 0, "bf16": 1, "f16": 2}


def test_struct_layouts_match_the_compiler(tmp_path):
    """sizeof and every offsetof as hipcc's host compiler lays the nine structs out, against the generated ctypes classes.  No GPU call."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "abi_layout_test"
    src = os.path.join(ROOT, "tests", "host", "abi_layout_test.hip")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", f"-I{os.path.join(ROOT, 'include')}", src, "-o", str(exe)],
                   check=True, timeout=600)  # fmt: skip
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    compiled = {key: int(value) for key, value in (line.split() for line in out.stdout.splitlines())}
    generated = {}
    for name in STRUCT_NAMES:
        cls = _hip.STRUCTS[name]
        generated[name] = ctypes.sizeof(cls)
        generated.update({f"{name}.{member}": getattr(cls, member).offset for member, _ in cls._fields_})
    assert compiled == generated


def _slots(struct):
    """{name: address or None} of every pointer slot of a struct, array slots as member + index; read without `_hip.fill`'s tables."""
    out = {}
    for member, t in struct._fields_:
        v = getattr(struct, member)
        if hasattr(t, "_length_"):
            out.update({f"{member}{i}": v[i] for i in range(t._length_)})
        else:
            out[member] = v if t is c_void_p else (ctypes.cast(v, c_void_p).value if v else None)
    return out


def test_fill_places_the_vrnn_parameters_where_the_struct_has_them():
    """The 28 VRNN parameters numbered 1 .. 28 in `_VRNN_PARAM_ORDER`: the struct's 28 pointer words, in memory order, written out."""
    assert (len(ops._VRNN_PARAM_ORDER), len(ops._SRNN_PARAM_ORDER), len(ops._RSSM_PARAM_ORDER)) == (28, 16, 22)
    for cls in (_hip.VrnnWeights, _hip.VrnnGrads):
        w = _hip.fill(cls(), ops._VRNN_PARAM_ORDER, range(1, 29))
        words = list((c_void_p * 28).from_buffer(w))
        assert ctypes.sizeof(w) == 28 * ctypes.sizeof(c_void_p)
        assert words == [1, 3, 5, 2, 4, 6, 7, 8] + [9, 11, 13, 10, 12, 14, 15, 16] + [17, 19, 21, 23, 18, 20, 22, 24] + [25, 26, 27, 28]
    assert ops._pack_weights([None] * 28).__class__ is _hip.VrnnWeights


DECODE_HEADS = lambda first: [f"{part}_{k}{i}" for part in (first, "dec") for i in range(3) for k in "wb"] + ["lik_w", "lik_b"]  # noqa: E731


@pytest.mark.parametrize(
    "cls, names, unnamed",
    [
        ("BlvmSrnnWeights", ops._SRNN_PARAM_ORDER, []),
        ("BlvmSrnnGrads", ops._SRNN_PARAM_ORDER, []),
        ("BlvmRssmWeights", ops._RSSM_PARAM_ORDER, []),
        ("BlvmRssmGrads", ops._RSSM_PARAM_ORDER, []),
        ("BlvmVrnnDecodeWeights", DECODE_HEADS("enc"), ["cell"]),
        ("BlvmSrnnDecodeWeights", DECODE_HEADS("enc") + ["gru_wih", "gru_whh", "gru_bih", "gru_bhh"], ["chain"]),
        ("BlvmLstmDecodeWeights", DECODE_HEADS("emb"), ["wih", "whh", "bih", "bhh"]),
    ],
)
def test_fill_reads_back_every_named_slot_and_leaves_the_rest_null(cls, names, unnamed):
    assert len(set(names)) == len(names)
    values = {name: 1000 + 7 * i for i, name in enumerate(names)}
    got = _slots(_hip.fill(_hip.STRUCTS[cls](), names, [values[n] for n in names]))
    assert got == {**values, **{n: None for n in unnamed}}
    # None stays NULL, and half the names leave the other half NULL
    half = list(names)[::2]
    got = _slots(_hip.fill(_hip.STRUCTS[cls](), half, [None if i == 0 else values[n] for i, n in enumerate(half)]))
    assert got == {n: (values[n] if n in half[1:] else None) for n in [*names, *unnamed]}


def test_fill_refuses_unknown_names_indices_past_the_end_and_uneven_lists():
    for name in ("prior_w3", "phi_w4", "prior_hw0", "prior_w", "prior", "gin_w", "prior_w-1", "prior_w 1", ""):
        w = _hip.VrnnWeights()
        with pytest.raises((_hip.BlvmHipError, TypeError)):
            _hip.fill(w, [name], [5])
        assert all(v is None for v in _slots(w).values()), name
    with pytest.raises(_hip.BlvmHipError, match="enc_w3"):
        _hip.fill(_hip.VrnnDecodeWeights(), ["enc_w3"], [5])
    with pytest.raises(ValueError):
        _hip.fill(_hip.SrnnWeights(), ops._SRNN_PARAM_ORDER, range(15))
