"""ctypes binding of libblvm_hip.so (the C ABI declared in include/blvm_hip.h).

No torch types cross this boundary: tensors are passed as raw device pointers (`tensor.data_ptr()`), sizes as ints,
the stream as the current torch HIP stream handle.  There is NO CPU fallback: every wrapper raises if the library
is missing or if it is handed a tensor that does not live on a HIP device.
"""
import ctypes
import functools
import os
import re

import torch

# BLVM_HIP_LIB: an alternative build of the same library (kernel experiments); the default is the in-tree build
_LIB_PATH = os.environ.get("BLVM_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libblvm_hip.so")
_lib = None


class BlvmHipError(RuntimeError):
    pass


# The header is the one declaration of the ABI: prototypes, structs and constants are read from it at import (pure text: no
# library, no GPU).  Found the way the Makefile's -I finds it.
_HEADER_PATH = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "include", "blvm_hip.h"))

_RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t}  # and const char*
_SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float, "double": ctypes.c_double,
            "size_t": ctypes.c_size_t, "long long": ctypes.c_longlong, "int32_t": ctypes.c_int32}  # fmt: skip
_POINTEE_WORDS = {"void", "char", "int", "unsigned", "long", "float", "double", "size_t", "int32_t"}
_STARS = r"((?:\*\s*(?:const\b\s*)?)*)"
_PROTOTYPE = re.compile(r"(int|size_t|const\s+char\s*\*)\s*(blvm_\w+)\s*\(([^()]*)\)")
_PARAM = re.compile(rf"(?:const\s+)?(\w+(?:\s+\w+)*?)\s*{_STARS}(\w+)\s*(\[\d*\])?")  # type words, stars, name, array
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;")
_MEMBERS = re.compile(r"(?:const\s+)?(\w+)\s*(\*.*)")  # pointee, declarators
_DECLARATOR = re.compile(rf"{_STARS}(\w+)\s*(?:\[(\d+)\])?")  # stars, name, array length
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(BLVM_\w+)[ \t]+(?:\((-?\d+)\)|(-?\d+))(?!\w)", re.M)


def parse_header(text):
    """The subset of C that include/blvm_hip.h is written in -> (structs {name: ctypes.Structure class}, signatures
    {name: (restype, argtypes)}, constants {name: int}).  Every pointer is a void* except a pointer to one of the header's structs.
    Anything outside the subset raises BlvmHipError quoting the declaration: nothing is guessed and nothing is skipped."""
    constants = {name: int(a or b) for name, a, b in _DEFINE.findall(text)}
    body = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    body = re.sub(r"^[ \t]*#.*$", "", body, flags=re.M)
    structs, signatures = {}, {}

    def bad(why, decl):
        return BlvmHipError(f"blvm_hip.h: {why}: {decl}")

    def pointer(words, stars, decl):
        if words in structs:
            return ctypes.POINTER(structs[words]) if stars == 1 else ctypes.c_void_p
        if not set(words.split()) <= _POINTEE_WORDS:
            raise bad(f"pointer to the unknown type {words!r}", decl)
        return ctypes.c_void_p

    def struct(m):
        decl = " ".join(m.group(0).split())
        name, members, alias = m.groups()
        if name != alias:
            raise bad("struct tag and typedef name differ", decl)
        fields = []
        for line in filter(None, (" ".join(s.split()) for s in members.split(";"))):
            mm = _MEMBERS.fullmatch(line)
            dms = [_DECLARATOR.fullmatch(d.strip()) for d in mm.group(2).split(",")] if mm else [None]
            if not all(dm and dm.group(1) for dm in dms) or (mm.group(1) != "float" and mm.group(1) not in structs):
                raise bad(f"member `{line}` is not pointers to float or to an earlier struct", decl)
            for stars, member, length in (dm.groups() for dm in dms):
                # a host array of device pointers (float *const *) keeps its pointee type
                t = ctypes.POINTER(ctypes.c_void_p) if stars.count("*") == 2 else pointer(mm.group(1), stars.count("*"), decl)
                fields.append((member, t * int(length) if length else t))
        structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields})
        return " "

    body = _STRUCT.sub(struct, body)
    body = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", body, flags=re.S)
    *decls, tail = (" ".join(s.split()) for s in body.split(";"))
    if tail:
        raise bad("a declaration without its `;`", tail)
    for decl in filter(None, decls):
        m = _PROTOTYPE.fullmatch(decl)
        if not m:
            raise bad("not `int | size_t | const char* blvm_name(parameters);` or `typedef struct Name {members} Name;`", decl)
        ret, name, params = m.groups()
        argtypes = []
        for p in [] if params.strip() in ("", "void") else [p.strip() for p in params.split(",")]:
            pm = _PARAM.fullmatch(p)
            if not pm:
                raise bad(f"parameter `{p}` is not `type name`", decl)
            words, stars = pm.group(1), pm.group(2).count("*") + bool(pm.group(4))
            if stars:
                argtypes.append(pointer(words, stars, decl))
            elif words in _SCALARS:
                argtypes.append(_SCALARS[words])
            else:
                raise bad(f"parameter `{p}` is passed by value and its type is none of {sorted(_SCALARS)}", decl)
        signatures[name] = (_RETURNS.get(ret, ctypes.c_char_p), argtypes)
    return structs, signatures, constants


try:
    with open(_HEADER_PATH) as _f:
        STRUCTS, SIGNATURES, CONSTANTS = parse_header(_f.read())
except OSError as e:
    raise BlvmHipError(f"the ABI header could not be read at {_HEADER_PATH}: {e}") from e

for _name, _cls in STRUCTS.items():  # a *Grads struct is filled in the Python-side order of its *Weights twin
    if _name.endswith("Grads") and _cls._fields_ != STRUCTS[_name[:-5] + "Weights"]._fields_:
        raise BlvmHipError(f"{_HEADER_PATH}: the members of {_name} differ from those of {_name[:-5]}Weights")

VrnnWeights, VrnnGrads, VrnnDecodeWeights = STRUCTS["BlvmVrnnWeights"], STRUCTS["BlvmVrnnGrads"], STRUCTS["BlvmVrnnDecodeWeights"]
SrnnWeights, SrnnGrads, SrnnDecodeWeights = STRUCTS["BlvmSrnnWeights"], STRUCTS["BlvmSrnnGrads"], STRUCTS["BlvmSrnnDecodeWeights"]
RssmWeights, RssmGrads, LstmDecodeWeights = STRUCTS["BlvmRssmWeights"], STRUCTS["BlvmRssmGrads"], STRUCTS["BlvmLstmDecodeWeights"]


@functools.lru_cache(maxsize=None)
def _slots(cls):
    """{slot name: (member, index)} of a struct class: a member under its own name (index None), every slot of an array member under
    the member's name followed by the decimal index (`prior_w2` is prior_w[2])."""
    slots = {}
    for member, t in cls._fields_:
        slots[member] = (member, None)
        for i in range(getattr(t, "_length_", 0)):
            slots[f"{member}{i}"] = (member, i)
    return slots


def fill(struct, names, addresses):
    """struct.<slot> = address for every (name, address) pair, slots named as in `_slots`.  None stays NULL.  A name that is no slot
    of the struct (an index past an array's end included) raises.  -> struct."""
    slots = _slots(type(struct))
    for name, address in zip(names, addresses, strict=True):
        if name not in slots:
            raise BlvmHipError(f"struct {type(struct).__name__} has no slot {name!r}")
        member, i = slots[name]
        if i is None:
            setattr(struct, member, address)
        else:
            getattr(struct, member)[i] = address
    return struct


def lib_path() -> str:
    return _LIB_PATH


def load():
    """Load libblvm_hip.so (once) and attach argument/return types.  Raises BlvmHipError if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise BlvmHipError(
                f"libblvm_hip.so not found at {_LIB_PATH}: build it with benchmarking-lvms_amd/csrc/build.sh "
                "(or __graft_entry__.build()).  There is no CPU/PyTorch fallback for the blvm hot path."
            )
        lib = ctypes.CDLL(_LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().blvm_last_error().decode(errors="replace")
        raise BlvmHipError(f"{what} failed (code {rc}): {msg}")


def take_async_errors():
    """(number of persistent launches of this process that gave up on a bounded spin since the previous take, code of the last one).
    Read-and-clear: an abort is reported once.  A read of pinned host memory — meaningful after the host has synchronised."""
    code = ctypes.c_uint(0)
    n = load().blvm_async_errors_take(ctypes.byref(code))
    return int(n), int(code.value)


def check_async(what: str = "a persistent recurrent launch", group=None):
    """Raise if a persistent chain launch of this process gave up on a bounded spin since the last check (its results are garbage).
    Cheap (a read of pinned host memory): called wherever the host has just synchronised with the device to read results back.
    With a `torch.distributed` process group (`group=True`: the default group) the count is all-reduced (MAX) first, so that every
    rank raises together instead of one rank leaving the others blocked in their next collective."""
    n, code = take_async_errors()
    local = n
    if group is not None and group is not False:
        import torch.distributed as dist

        if dist.is_available() and dist.is_initialized():
            pg = None if group is True else group
            on_gpu = dist.get_backend(pg) == "nccl"
            t = torch.tensor([n], dtype=torch.int32, device="cuda" if on_gpu else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=pg)
            n = int(t.item())
    if n:
        where = f"last at step {code >> 4}, link {code & 15}" if local else "on another rank"
        raise BlvmHipError(
            f"{what}: {n} persistent launch(es) aborted on a bounded spin ({where}): "
            "a workgroup of the launch was not resident (is another process using this GPU?); results are invalid"
        )


DTYPES = {"f32": CONSTANTS["BLVM_DTYPE_F32"], "bf16": CONSTANTS["BLVM_DTYPE_BF16"], "f16": CONSTANTS["BLVM_DTYPE_F16"]}


def set_operand_dtype(name: str):
    """Operand type of the matrix products: "f32" (default), "bf16" or "f16" (16-bit operands rounded to nearest even, fp32
    accumulation, for the persistent recurrent chains, the sequence and WaveNet block kernels and the K6 GEMMs) — what the reference's
    `--use_amp True` selects with torch.autocast (`experiments/experiment_vrnn_audio.py:219-230`; autocast's type is fp16, whose
    gradients need loss scaling: torch.amp.GradScaler).  Process-wide."""
    if name not in DTYPES:
        raise ValueError(f"operand dtype {name!r}: one of {sorted(DTYPES)}")
    check(load().blvm_set_operand_dtype(DTYPES[name]), "blvm_set_operand_dtype")


def get_operand_dtype() -> str:
    v = load().blvm_get_operand_dtype()
    for name, code in DTYPES.items():
        if code == v:
            return name
    raise BlvmHipError(f"blvm_get_operand_dtype: unknown operand type {v}")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def stream_ptr() -> int:
    """hipStream_t of torch's current stream on the current device, as an integer.  Through the raw accessors when this torch has
    them (0.1 us; `torch.cuda.current_stream().cuda_stream` builds a Stream object per call: 2.7 us, a third of a small launch's host
    cost — the CW-VAE step makes ~1 000 such calls)."""
    if _raw_stream is not None and _raw_device is not None:
        return _raw_stream(_raw_device())
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    """Device pointer of a tensor (None -> NULL).  Refuses anything that is not a contiguous HIP tensor."""
    if t is None:
        return None
    if not t.is_cuda:
        raise BlvmHipError(
            "blvm HIP kernels were handed a CPU tensor: this build runs the hot path on gfx950 only "
            "(no CPU fallback); move the model and inputs to a HIP device."
        )
    if not t.is_contiguous():
        raise BlvmHipError("blvm HIP kernels need contiguous tensors")
    return t.data_ptr()
