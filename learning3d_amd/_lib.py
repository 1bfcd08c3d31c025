"""ctypes binding of libl3d_hip.so (the C ABI declared in include/*.h: l3d_hip.h and one header per later model; models added
after the table of include/*.h was closed declare theirs in include/models/*.h, read the same way into MODEL_PROTOTYPES).
Both of those tables are pinned by tests.  include/ext/*.h is the third and the OPEN one (EXT_PROTOTYPES, EXT_SIGNATURES,
EXT_CONSTANTS): a new model adds its header there, and nothing pins that table's size or contents.

The headers are the one description of that boundary: the prototypes, the integer #defines and the l3d_status enum are parsed
from them when this module is imported (SIGNATURES, PROTOTYPES, CONSTANTS), and `call` is the one launch path built on them.

The product path has NO fallback: if the shared library is missing, fails to load, or a call
returns a non-zero status, this module raises.  PyTorch is used only for device memory
(`tensor.data_ptr()`), streams (`torch.cuda.current_stream()`) and torch.distributed.
"""
import ctypes as C
import glob
import os
import re
from collections import namedtuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# L3D_LIB_PATH: a library built from the same sources with other -D flags (tools/build_variant_lib.py: A/B runs of bench.py on one box)
LIB_PATH = os.environ.get("L3D_LIB_PATH") or os.path.join(_HERE, "libl3d_hip.so")
INCLUDE_DIR = os.path.join(_HERE, "..", "include")
_lib = None


class L3DError(RuntimeError):
    pass


# ------------------------------------------------------------------------------------------------------------
# The headers -> prototypes.  A small, strict parser of the C the headers actually use; anything else raises.
_SCALAR = {"int": C.c_int, "unsigned": C.c_uint, "long": C.c_long, "long long": C.c_longlong, "unsigned long long": C.c_ulonglong,
           "size_t": C.c_size_t, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double,
           "l3d_stream_t": C.c_void_p}
# element type of a pointer parameter -> the dtype a tensor passed for it must have (None: any)
_ELEMENT = {"float": torch.float32, "double": torch.float64, "int32_t": torch.int32, "int": torch.int32, "unsigned": torch.int32,
            "int64_t": torch.int64, "long long": torch.int64, "long": torch.int64, "void": None, "char": None, "unsigned char": None}
_PARAM = re.compile(r"(?:const\s+)?(?P<base>[a-z0-9_]+(?: [a-z0-9_]+)*?)\s*(?P<ptr>\*\s*(?:const\s+)?)?(?P<name>\w+)\s*(?P<arr>\[\d*\])?")
_RETURN = re.compile(r"(?:const\s+)?(?P<base>[a-z0-9_]+(?: [a-z0-9_]+)*?)\s*(?P<ptr>\*)?")

_Tensor = torch.Tensor
_NOT_TENSORS = {int, float, bool, type(None)}     # `call`: argument types already seen not to be tensors
_BY_VALUE, _POINTERS = object(), object()         # `call`: parameters that take no tensor, beside the dtypes of _ELEMENT
# a parameter: its C type as written (`st[4]` as `[]`), its name, the base type, and 0 = by value, 1 = pointer / array, 2 = pointer array
Param = namedtuple("Param", "ctype name element indirection")
Prototype = namedtuple("Prototype", "restype params")      # restype: a ctypes type; params: tuple of Param


def _blank(m):
    return "\n" * m.group().count("\n")                              # cut text, keep the line numbers


def parse_header(text, where="<header>"):
    """-> ({name: Prototype}, {NAME: int}) of one header's `ret l3d_name(params);` declarations, `#define NAME <int>` lines and
    l3d_status enumerators.  An unknown type or a declaration of another shape raises L3DError with the header line."""
    text = re.sub(r"/\*.*?\*/", _blank, text, flags=re.S)
    consts = {n: int(v, 0) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(-?(?:0x[0-9a-fA-F]+|\d+))[ \t]*$", text, flags=re.M)}
    text = re.sub(r"^[ \t]*#ifdef __cplusplus\n.*?^[ \t]*#endif[ \t]*$", _blank, text, flags=re.S | re.M)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)

    def fail(pos, what):
        raise L3DError(f"{where}:{text.count(chr(10), 0, pos) + 1}: {what}")

    def c_type(pattern, decl, pos):
        m = pattern.fullmatch(decl)
        if m is None or m["base"] not in (_ELEMENT if m["ptr"] or m.groupdict().get("arr") else _SCALAR):
            fail(pos, f"unrecognised C type in {decl!r}")
        return m

    protos, pos = {}, 0
    for stmt in text.split(";"):
        start, pos = pos + len(stmt) - len(stmt.lstrip()), pos + len(stmt) + 1
        stmt = " ".join(stmt.split())
        enum = re.fullmatch(r"typedef enum \{(.*)\} l3d_status", stmt)
        if enum:
            consts.update({n: int(v, 0) for n, v in re.findall(r"(\w+) = (-?\w+)", enum[1])})
        if "(" not in stmt:
            continue
        decl = re.fullmatch(r"(.*?)\b(l3d_\w+) ?\((.*)\)", stmt)
        if decl is None:
            fail(start, f"not a `ret l3d_name(params)` declaration: {stmt!r}")
        ret = c_type(_RETURN, decl[1].strip(), start)
        params = []
        for p in ([] if decl[3].strip() == "void" else [p.strip() for p in decl[3].split(",")]):
            m = c_type(_PARAM, p, start)
            params.append(Param(p[:m.start("name")].strip() + ("[]" if m["arr"] else ""), m["name"], m["base"], bool(m["ptr"]) + bool(m["arr"])))
        restype = (C.c_char_p if ret["base"] == "char" else C.c_void_p) if ret["ptr"] else _SCALAR[ret["base"]]
        protos[decl[2]] = Prototype(restype, tuple(params))
    return protos, consts


def _parse_headers(directory):
    """-> ({name: Prototype}, {NAME: int}) of every *.h in `directory`; an entry point declared by two headers, or a constant they
    give two values, raises, naming both"""
    protos, consts, declared_in = {}, {}, {}
    for path in sorted(glob.glob(os.path.join(directory, "*.h"))):
        where = os.path.basename(path)
        with open(path) as f:
            p, c = parse_header(f.read(), where)
        for name in p:
            if name in protos:
                raise L3DError(f"{name} is declared by {declared_in[name]} and by {where}")
        for name, value in c.items():
            if consts.get(name, value) != value:
                raise L3DError(f"{name} is {consts[name]} in {declared_in[name]} and {value} in {where}")
        declared_in.update(dict.fromkeys((*p, *c), where))
        protos.update(p)
        consts.update(c)
    return protos, consts


PROTOTYPES, CONSTANTS = _parse_headers(INCLUDE_DIR)   # name -> Prototype; L3D_* #defines and l3d_status enumerators -> int
globals().update(CONSTANTS)                        # _lib.L3D_OK, _lib.L3D_CONV_F16_TWO_PLANE, _lib.L3D_SELF_ATTN_TQ, ...
SIGNATURES = {name: [_SCALAR[p.element] if p.indirection == 0 else C.c_void_p for p in proto.params]
              for name, proto in PROTOTYPES.items()}                                                  # name -> argtypes
# include/models/*.h: the same parser and the same launch path; a name or constant include/*.h already has raises
MODEL_PROTOTYPES, MODEL_CONSTANTS = _parse_headers(os.path.join(INCLUDE_DIR, "models"))
for _name in MODEL_PROTOTYPES:
    if _name in PROTOTYPES:
        raise L3DError(f"{_name} is declared under include/ and again under include/models/")
for _name, _value in MODEL_CONSTANTS.items():
    if _name in CONSTANTS and CONSTANTS[_name] != _value:
        raise L3DError(f"{_name} is {CONSTANTS[_name]} under include/ and {_value} under include/models/")
globals().update(MODEL_CONSTANTS)                  # _lib.L3D_RRI_MAX_K, _lib.L3D_GMM_MAX_J
MODEL_SIGNATURES = {name: [_SCALAR[p.element] if p.indirection == 0 else C.c_void_p for p in proto.params]
                    for name, proto in MODEL_PROTOTYPES.items()}
# include/ext/*.h: the open table (RPMNet and later models); a name or constant that either earlier table has raises
EXT_PROTOTYPES, EXT_CONSTANTS = _parse_headers(os.path.join(INCLUDE_DIR, "ext"))
for _name in EXT_PROTOTYPES:
    if _name in PROTOTYPES or _name in MODEL_PROTOTYPES:
        raise L3DError(f"{_name} is declared under include/ext/ and again in an earlier header table")
for _name, _value in EXT_CONSTANTS.items():
    if _name in CONSTANTS or _name in MODEL_CONSTANTS:
        raise L3DError(f"{_name} is defined under include/ext/ and again in an earlier header table")
globals().update(EXT_CONSTANTS)                    # _lib.L3D_PPF_MAX_K, _lib.L3D_GN_CONV_MAX_COUT, ...
EXT_SIGNATURES = {name: [_SCALAR[p.element] if p.indirection == 0 else C.c_void_p for p in proto.params]
                  for name, proto in EXT_PROTOTYPES.items()}
_TABLES = ((PROTOTYPES, SIGNATURES), (MODEL_PROTOTYPES, MODEL_SIGNATURES), (EXT_PROTOTYPES, EXT_SIGNATURES))


def _declared(name):
    """-> (Prototype, argtypes) of an entry point, from whichever header table declares it"""
    for protos, sigs in _TABLES:
        if name in protos:
            return protos[name], sigs[name]
    raise L3DError(f"{name} is declared by no header")


_CALLS = {}                                        # name -> what `call` needs of an entry point; filled by lib()


def lib():
    """Load libl3d_hip.so once.  Raises (never falls back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise L3DError(
                f"{LIB_PATH} not found: build the HIP extension first "
                "(python -m learning3d_amd.build, or __graft_entry__.build()). "
                "learning3d_amd has no CPU / eager fallback by design.")
        handle = C.CDLL(LIB_PATH)
        for name in [n for protos, _ in _TABLES for n in protos]:
            proto, argtypes = _declared(name)
            fn = getattr(handle, name)          # AttributeError if the ABI drifted
            fn.argtypes = argtypes
            fn.restype = proto.restype
            # what `call` wants of a tensor passed for each parameter, worked out once: a dtype (pointer to that element type), None
            # (pointer to anything), or that there is none: _POINTERS (a pointer array: ctypes values only), _BY_VALUE
            wants = tuple(_BY_VALUE if p.indirection == 0 else _POINTERS if p.indirection == 2 else _ELEMENT[p.element] for p in proto.params)
            _CALLS[name] = (fn, wants, bool(proto.params) and proto.params[-1].element == "l3d_stream_t")
        _lib = handle
    return _lib


LAUNCH_LOG = None      # set to a list to record the name of every C-ABI call that passes through check() (tests: which route ran)
FAILED_CALLS = 0       # number of C-ABI calls that returned a non-zero status (holders of cross-call device state re-arm on a change)


def check(status, what):
    if LAUNCH_LOG is not None:
        LAUNCH_LOG.append(what)
    if status != 0:
        global FAILED_CALLS
        FAILED_CALLS += 1
        l = lib()
        msg = l.l3d_status_string(status).decode()
        raise L3DError(f"{what}: {msg} (status {status}, hipError {l.l3d_last_hip_error()})")


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Built(tuple):
    """(device index, raw stream, event) of a cache entry.  Entries live in module __dict__s, which copy.deepcopy and pickle walk, and
    an event can be neither copied nor pickled: a deep copy stands behind the copies of the entry's tensors (made on the current
    stream just before: the mark is the entry's last element), an unpickled one knows of no build."""
    __slots__ = ()

    def __deepcopy__(self, memo):
        if not torch.cuda.is_available() or torch.cuda.is_current_stream_capturing():
            return _Built((self[0], None, None))
        event = torch.cuda.Event()
        event.record(torch.cuda.current_stream(self[0]))
        return _Built((self[0], torch._C._cuda_getCurrentRawStream(self[0]), event))

    def __reduce__(self):
        return (_Built, ((self[0], None, None),))


def built_on(t):
    """What a process-wide cache remembers of a device tensor it has just ENQUEUED the build of: (device index, the raw stream the
    build was put on, an event recorded behind it); None for a host tensor.  Under a capture no event is recorded (an event
    recorded inside a capture cannot be waited for outside it): a cache filled during a capture orders nothing across streams."""
    if t is None or not t.is_cuda:
        return None
    index = t.get_device()
    raw = torch._C._cuda_getCurrentRawStream(index)
    if torch.cuda.is_current_stream_capturing():
        return _Built((index, raw, None))
    event = torch.cuda.Event()
    event.record(torch.cuda.current_stream(index))
    return _Built((index, raw, event))


def order_after_build(mark):
    """A cache hit: on the stream the entry was built on, one comparison and nothing else -- no event call, no launch.  On any other
    stream the current stream waits for the build (the tensor was enqueued there, not necessarily written yet); while capturing it
    does not (a wait on an outside event would enter the graph: warm up on the capture's stream, or join, before capturing)."""
    if mark is not None and torch._C._cuda_getCurrentRawStream(mark[0]) != mark[1]:
        if mark[2] is not None and not torch.cuda.is_current_stream_capturing():
            torch.cuda.current_stream(mark[0]).wait_event(mark[2])


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def require_gpu(*tensors):
    """Device tensors only, all on ONE device, which must be the current device: the C ABI launches on the current
    device's current stream (stream_ptr), so a tensor living elsewhere would be read through a foreign pointer.  Raises
    instead (callers switch with `with torch.cuda.device(t.device):`)."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise L3DError("learning3d_amd operates on MI355X device tensors only "
                           "(got a CPU tensor; there is no CPU fallback)")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise L3DError(f"tensors on different devices in one call ({dev} and {t.device})")
    if dev is not None and dev.index != torch.cuda.current_device():
        raise L3DError(f"tensors live on {dev} but the current device is cuda:{torch.cuda.current_device()}; "
                       f"wrap the call in `with torch.cuda.device({dev.index}):`")


class on_device_of:
    """`with on_device_of(t, ...):` -- make the first device tensor's GPU the current device for the calls inside (the C ABI
    launches on the current device's current stream).  A no-op when it already is, or when no tensor is a device tensor."""

    def __init__(self, *tensors):
        self.dev = next((t.device for t in tensors if isinstance(t, torch.Tensor) and t.is_cuda), None)
        self.ctx = None

    def __enter__(self):
        if self.dev is not None and self.dev.index != torch.cuda.current_device():
            self.ctx = torch.cuda.device(self.dev)
            self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)
        return False


def f32c(t):
    """contiguous fp32 view/copy of a device tensor"""
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def f32a(t):
    """f32c(t) on a 16-byte boundary: a contiguous slice of a larger buffer (x[1:], a chunk of a flat tensor) is a legal input whose
    data pointer is only 4-byte aligned, and the entry points that read their operand 16 bytes at a time without a scalar route
    refuse it (L3D_ERR_UNSUPPORTED).  Their wrappers pass the operand through here: a copy when it is misaligned, t itself else."""
    t = f32c(t)
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def _bad_argument(name, i, a, want):
    p = _declared(name)[0].params[i]
    decl = p.ctype + ("" if p.ctype.endswith("*") else " ") + p.name
    if not p.indirection:
        return L3DError(f"{name}: parameter `{decl}` is passed by value, got a tensor")
    if want is _POINTERS:
        return L3DError(f"{name}: parameter `{decl}` takes a ctypes pointer array, got a tensor")
    return L3DError(f"{name}: parameter `{decl}` takes a {want} tensor, got {a.dtype}")


def call(name, *args, tag="", span=None):
    """THE launch path: l3d_<name>(*args) on the current device's current stream, status through check() under the label name + tag.
    Per pointer parameter: None -> NULL; a ctypes value or array -> as it is; a tensor -> its data pointer, after its dtype has
    been held against the parameter's element type in the header (float * takes float32, int32_t * int32, void * anything, ...).
    Then the tensors go through require_gpu (entry points without a stream parameter launch nothing and work on host memory: no
    device rule for them).  The trailing l3d_stream_t is filled in unless given.  span: a context manager entered around the
    library call alone (a timing span: the argument handling stays outside it)."""
    if _lib is None:
        lib()
    fn, wants, has_stream = _CALLS[name]
    if len(args) != len(wants) and len(args) + has_stream != len(wants):
        raise L3DError(f"{name}: takes {len(wants)} arguments{' (the stream may be left out)' if has_stream else ''}, got {len(args)}")
    out, dev, same = list(args), None, True
    for i, a in enumerate(args):
        t = type(a)
        if t is not _Tensor:
            # isinstance() of a non-tensor is the slow path of torch's metaclass: each other type (int, None, a ctypes array) pays it once
            if t in _NOT_TENSORS:
                continue
            if not isinstance(a, _Tensor):
                _NOT_TENSORS.add(t)
                continue
        want = wants[i]
        if a.dtype is not want and want is not None:
            raise _bad_argument(name, i, a, want)
        out[i] = a.data_ptr()
        if dev is None:
            dev = a.get_device()                                        # the GPU's index, -1 for a CPU tensor
        elif a.get_device() != dev:
            same = False
    if has_stream:
        if dev is not None and (dev < 0 or not same):
            require_gpu(*[a for a in args if isinstance(a, _Tensor)])   # its rule, seen to be broken: it raises, with its messages
        if len(args) < len(wants):
            stream = torch.cuda.current_stream()
            current = stream.device_index
            out.append(stream.cuda_stream)
        else:
            current = torch.cuda.current_device() if dev is not None else None
        if dev is not None and dev != current:
            require_gpu(*[a for a in args if isinstance(a, _Tensor)])
    if span is None:
        status = fn(*out)
    else:
        with span:
            status = fn(*out)
    check(status, name + tag)
