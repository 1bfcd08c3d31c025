"""The memory side of the C ABI, as the headers state it: which pointer parameters a launch may write (everything `_lib.PROTOTYPES`
does not mark `const`), and for each of those whether it is FULLY WRITTEN (the default), IN-OUT with a precondition, or SCRATCH --
plus the size function that governs a workspace or a packed image and the bytes of an output the header leaves open.

CONTRACT holds only what the headers say in prose; a writable parameter without an entry is "fully written".  A new entry point
registers here (if it has anything but fully written outputs) and gets a case in tests/test_gpu_memory_contract.py.

Arena gives every writable tensor of a call its own buffer of exactly the declared size between two guards of GUARD bytes, the
slice 256-byte aligned as the caching allocator's blocks are (the same vector routes as the product), pre-filled with 0xFF
(fill A: fp32 NaN, int -1) or 0x00 (fill B).  check() runs one call under both fills and asserts
  (a) every guard byte is intact,
  (b) every `const` tensor is bit for bit what it was,
  (c) every writable non-scratch tensor agrees bit for bit between the two runs outside its don't-care bytes
-- (c) fails for an element never written, a value read before it is written, and a result that depends on what a workspace held.
Both fills keep a stale value used as an index (-1, 0) inside the guards."""
import ctypes
from collections import namedtuple

import torch

GUARD = 4096
ALIGN = 256
FILL_A, FILL_B, GUARD_BYTE = 0xFF, 0x00, 0x5A
FILLS = (("A", FILL_A), ("B", FILL_B))


class ContractError(AssertionError):
    """a launch broke the memory contract of its entry point"""


# Hooks for a second way of running the same cases (tests/golden/stream_cases.py sets and resets them, a context manager each):
# DEFAULT_LAUNCH: what check() launches through when a case passes no `launch` (None: `_lib.call`).  ACTIVE is, for the time of one
# check(), what such a launch needs besides its arguments: (name, proto, contract, sizefn).
# RECORD: a list to which check() appends (name, values, {parameter: (clone of the tensor, spec)}) of its fill-B run.
DEFAULT_LAUNCH = None
ACTIVE = None
RECORD = None


# One writable parameter.  kind: "written" | "inout" | "scratch".  size: None, or (size function, args(v) -> tuple, bytes per unit)
# with v = {parameter name: the call's argument}; a size function given as a callable is called as it is (the ball-query formula).
# keep: bytes at the front of a scratch area that carry state from call to call ("zero before the first call, the kernel re-arms
# them"): check() runs a third time on the area the second run left.  open(v, nbytes) -> [(first byte, end byte)]: don't-care ranges.
# quote: the header's words.
# inout_when(v): the parameter is in-out only for these calls, fully written for the others.  bound(v) -> a tensor of the output's
# shape: the entry point is ORDER-DEPENDENT by its header (quote must be that line) and two runs may differ by at most this much.
Spec = namedtuple("Spec", "kind quote size keep open inout_when bound", defaults=(None, 0, None, None, None))


def _image_tail(v, nbytes):
    """an activation image is "h | m' planes + 16 bytes: 2^-T, scratch": the 12 bytes behind the scale are scratch"""
    return [(nbytes - 12, nbytes)]


def _act_image(rows, cols):
    return ("l3d_f16_image_bytes", lambda v: (1, rows(v), cols(v)), 1)


def _mask_select_open(what):
    """k == 0: "of which the first count[0] entries are written" -- the rest is open; count is read from the run itself"""
    def open_(v, nbytes, count=None):
        if int(v["k"]) > 0 or count is None:
            return []
        return [(int(count) * what, nbytes)]
    return open_


def _weight_image_pad(rows, cols, nbytes):
    """a weight image ends in "2^-S_r per row r ..., the list padded to a multiple of 16 bytes (the padding is SCRATCH)" """
    from learning3d_amd import _lib
    pb = int(_lib.lib().l3d_f16_image_bytes(0, rows, cols))
    return pb, [(3 * pb + 16 + 4 * rows, nbytes)]


def _operand_open(v, nbytes):
    """kind 0: an activation image; kind 1: "its Hs slot, the second plane, is NOT written" """
    if int(v["kind"]) == 0:
        return _image_tail(v, nbytes)
    pb, pad = _weight_image_pad(int(v["rows"]), int(v["C"]), nbytes)
    return [(pb, 2 * pb)] + pad


def _scatter_bound(src, idx, weight, T, div):
    """two fp32 sums of the same k terms in different orders differ by at most 2 (k - 1) 2^-24 sum |term| (each is within
    (k - 1) 2^-24 sum |term| of the exact sum); src [B,C,E/div], idx [B,E], weight [B,E] or None -> [B,C,T]"""
    def bound(v):
        s, ix = v[src].double().abs(), v[idx].long()
        B, Cc = s.shape[0], s.shape[1]
        s, ix = s.reshape(B, Cc, -1), ix.reshape(B, -1)
        terms = s.repeat_interleave(div, dim=2)
        if weight is not None:
            terms = terms * v[weight].double().abs().reshape(B, 1, -1)
        Tn = int(v[T])
        total = torch.zeros(B, Cc, Tn, dtype=torch.float64, device=s.device).scatter_add_(2, ix[:, None, :].expand(B, Cc, -1), terms)
        count = torch.zeros(B, 1, Tn, dtype=torch.float64, device=s.device).scatter_add_(2, ix[:, None, :], torch.ones_like(ix[:, None, :], dtype=torch.float64))
        return 2.0 * (count - 1).clamp_min(0) * 2.0 ** -24 * total
    return bound


ORDER_DEPENDENT = "ORDER-DEPENDENT, like the reference's kernel: an fp32 atomicAdd scatter"

RANGE_FLAG = Spec("inout", "stores 1 to *range_flag ... when a plane value exceeds 60000: sticky, the caller zeroes it")

CONTRACT = {
    "l3d_probe_mfma_sustained": {"sink": Spec("scratch", "sink: 131 072 floats of SCRATCH"),
                                 "ticks": Spec("written", "two timer readings: they differ from run to run", open=lambda v, nbytes: [(0, nbytes)])},
    "l3d_group_points_grad": {"grad_points": Spec("written", ORDER_DEPENDENT, bound=_scatter_bound("grad_out", "idx", None, "n", 1))},
    "l3d_gather_points_grad": {"grad_points": Spec("written", ORDER_DEPENDENT, bound=_scatter_bound("grad_out", "idx", None, "n", 1))},
    "l3d_three_interpolate_grad": {"grad_points": Spec("written", ORDER_DEPENDENT, bound=_scatter_bound("grad_out", "idx", "weight", "m", 3))},
    "l3d_scatter_add_det": {"workspace": Spec("scratch", "workspace: >= l3d_scatter_add_det_workspace_bytes(B,T,E) bytes",
                                              ("l3d_scatter_add_det_workspace_bytes", lambda v: (v["B"], v["T"], v["E"]), 1))},
    "l3d_knn_feature": {"workspace": Spec("scratch", "workspace: >= l3d_knn_feature_workspace_bytes(B,C,N) bytes",
                                          ("l3d_knn_feature_workspace_bytes", lambda v: (v["B"], v["C"], v["N"]), 1))},
    "l3d_chamfer_loss_local_mb": {"ws": Spec("scratch", "first 8 bytes are zero before the first call (the kernel re-arms them)",
                                             ("l3d_chamfer_loss_local_ws_bytes", lambda v: (), 1), keep=8)},
    "l3d_chamfer_forward_loss": {"ws": Spec("scratch", "the first 16 zero before the first call (the kernel re-arms them)",
                                            ("l3d_chamfer_forward_loss_ws_bytes", lambda v: (v["B"], v["N"], v["M"]), 1), keep=16)},
    "l3d_chamfer_forward_grid_stats": {"stats": Spec("inout", "stats: 3 int32 on the device, zeroed by the caller")},
    "l3d_ball_query": {"workspace": Spec("scratch", "NULL, or b * (16 n + 16448) bytes of device scratch",
                                         (lambda b, n: b * (16 * n + 16448), lambda v: (v["b"], v["n"]), 1))},
    "l3d_furthest_point_sampling": {"temp": Spec("scratch", "temp [B,n] scratch (callee initialises it to 1e10)")},
    "l3d_farthest_point_sample": {"temp": Spec("scratch", "temp [B,N] scratch")},
    "l3d_soft_correspondence": {"workspace": Spec("scratch", "scratch of l3d_soft_correspondence_workspace_floats(B,N,M) floats",
                                                  ("l3d_soft_correspondence_workspace_floats", lambda v: (v["B"], v["N"], v["M"]), 4))},
    "l3d_attention_forward_f16b": {
        "workspace": Spec("scratch", ">= 16 bytes of device memory, contents irrelevant (maxima_ready bit 0: the caller's maxima)",
                          (lambda: 16, lambda v: (), 1)),
        "ctx_img": Spec("written", "l3d_f16_image_bytes(1, B N, H D) bytes", _act_image(lambda v: v["B"] * v["N"], lambda v: v["H"] * v["D"]),
                        open=_image_tail)},
    "l3d_layernorm_planes": {"img": Spec("written", "l3d_f16_image_bytes(1, rows, C) bytes", _act_image(lambda v: v["rows"], lambda v: v["C"]),
                                         open=_image_tail)},
    "l3d_layernorm_planes_cf": {"img": Spec("written", "img: l3d_f16_image_bytes(1, B N, C) bytes",
                                            _act_image(lambda v: v["B"] * v["N"], lambda v: v["C"]), open=_image_tail)},
    "l3d_edgeconv_forward_f16b": {"range_flag": RANGE_FLAG},      # `out` is fp32 or an image by out_mode: sized by the case
    "l3d_edgeconv_pack": {"packed": Spec("written", "Number of floats of the packed EdgeConv parameter block",
                                         ("l3d_edgeconv_packed_floats", lambda v: (v["c1"], v["c2"], v["c3"], v["c4"]), 4))},
    "l3d_group_first_layer_planes_auto": {
        "out_img": Spec("written", "the activation image of [B S K][C1]", _act_image(lambda v: v["B"] * v["S"] * v["K"], lambda v: v["C1"]),
                        open=_image_tail),
        "range_flag": RANGE_FLAG},
    "l3d_split_rows": {"dst": Spec("written", "l3d_split_bytes(rows, cols)", ("l3d_split_bytes", lambda v: (v["rows"], v["cols"]), 1))},
    "l3d_conv_f16_split_weights": {"dst": Spec("written", "kind 2: a split weight image of [rows = Cout][cols = Cin]",
                                               ("l3d_f16_image_bytes", lambda v: (2, v["Cout"], v["Cin"]), 1),
                                               open=lambda v, nbytes: _weight_image_pad(int(v["Cout"]), int(v["Cin"]), nbytes)[1])},
    "l3d_split_f16_rows": {"dst": Spec("written", "-> activation image", _act_image(lambda v: v["rows"], lambda v: v["C"]), open=_image_tail),
                           "range_flag": RANGE_FLAG},
    "l3d_split_f16_operand": {
        "dst": Spec("written", "kind 0: l3d_f16_image_bytes(1, rows, C); kind 1: l3d_f16_image_bytes(2, rows, C)",
                    ("l3d_f16_image_bytes", lambda v: (1 + v["kind"], v["rows"], v["C"]), 1),
                    open=_operand_open),
        "range_flag": RANGE_FLAG},
    "l3d_first_layer_f16_planes": {
        "out_img": Spec("written", "written straight as an activation image", _act_image(lambda v: v["B"] * v["N"], lambda v: v["Cout"]),
                        open=_image_tail),
        "range_flag": RANGE_FLAG},
    "l3d_pointwise_conv_f16": {
        "out_img": Spec("written", "l3d_f16_image_bytes(1, B N, Cout) bytes", _act_image(lambda v: v["B"] * v["N"], lambda v: v["Cout"]),
                        open=_image_tail),
        "amax_out": Spec("inout", "uint32 float bits, atomic maximum: the caller zeroes them first")},
    "l3d_emd_forward": {"workspace": Spec("scratch", "l3d_emd_workspace_bytes(B,n,m) bytes ... no initialisation needed",
                                          ("l3d_emd_workspace_bytes", lambda v: (v["B"], v["n"], v["m"]), 1))},
    "l3d_bn_finalize": {"running_mean": Spec("inout", "running statistics updated as torch.nn.BatchNorm does when given"),
                        "running_var": Spec("inout", "running statistics updated as torch.nn.BatchNorm does when given")},
    "l3d_layernorm_ref_backward": {"workspace": Spec("scratch", "l3d_layernorm_backward_workspace_floats(rows, C) floats",
                                                     ("l3d_layernorm_backward_workspace_floats", lambda v: (v["rows"], v["C"]), 4))},
    "l3d_bmm_f32": {"C": Spec("inout", "C is IN-OUT with flag 1, fully written without it", inout_when=lambda v: bool(int(v["flags"]) & 1)),
                    "workspace": Spec("scratch", "`workspace` (nb1 nb2 parts M N floats)",
                                      (lambda nb1, nb2, parts, M, N: nb1 * nb2 * parts * M * N, lambda v: (v["nb1"], v["nb2"], v["parts"], v["M"], v["N"]), 4))},
    "l3d_colsum_rows": {"workspace": Spec("scratch", "workspace: l3d_colsum_rows_workspace_bytes",
                                          ("l3d_colsum_rows_workspace_bytes", lambda v: (v["rows"], v["cols"]), 1))},
    "l3d_wgrad": {"workspace": Spec("scratch", "workspace: l3d_wgrad_workspace_bytes(B, Cout, Cin, P, pc) bytes",
                                    ("l3d_wgrad_workspace_bytes", lambda v: (v["B"], v["Cout"], v["Cin"], v["P"], v["pc"]), 1))},
    "l3d_mask_select": {"idx": Spec("written", "k == 0: the first count[0] entries are written", open=_mask_select_open(8)),
                        "out": Spec("written", "k == 0: the first count[0] entries are written", open=_mask_select_open(12))},
    "l3d_reg_jac_pinv": {"singular": Spec("inout", "singular: int32 [1 + B], zeroed by the caller")},
    "l3d_reg_iclk_step": {"ws": Spec("scratch", "ws: fp32 [B,8] scratch"),
                          "state": Spec("inout", "state: int32 [4] ... zeroed by the caller once"),
                          "est_T": Spec("inout", "Launch 0 takes est_T = identity; later launches update it"),
                          "series": Spec("inout", "a launch fills its slot of est_T_series (launch 0: slots 0 and 1)"),
                          "r": Spec("inout", "once done is set a launch leaves r as it is")},
    "l3d_reg_quat_update": {"est_R": Spec("inout", "est_R <- R_q est_R (first != 0: not read, fully written)"),
                            "est_t": Spec("inout", "est_t <- R_q est_t + t_q (first != 0: not read, fully written)")},
}

# exported, described in l3d_hip_testing.h and deliberately not declared: bound by name, its parameters spelled here
GRID_STATS = "l3d_chamfer_forward_grid_stats"
GRID_STATS_PARAMS = (("const float *", "xyz1", "float", 1), ("const float *", "xyz2", "float", 1), ("int", "B", "int", 0), ("int", "N", "int", 0),
                     ("int", "M", "int", 0), ("float *", "dist1", "float", 1), ("float *", "dist2", "float", 1), ("int32_t *", "idx1", "int32_t", 1),
                     ("int32_t *", "idx2", "int32_t", 1), ("int32_t *", "stats", "int32_t", 1), ("l3d_stream_t", "stream", "l3d_stream_t", 0))


def prototypes():
    """name -> Prototype of every entry point: the two header tables and the grid-stats kernel"""
    from learning3d_amd import _lib
    protos = {**_lib.PROTOTYPES, **_lib.MODEL_PROTOTYPES}
    protos[GRID_STATS] = _lib.Prototype(ctypes.c_int, tuple(_lib.Param(*p) for p in GRID_STATS_PARAMS))
    return protos


def is_writable(p):
    return p.indirection >= 1 and not p.ctype.startswith("const")


def has_stream(proto):
    return any(p.element == "l3d_stream_t" for p in proto.params)


def spec_of(name, param, contract=None):
    return (CONTRACT if contract is None else contract).get(name, {}).get(param) or Spec("written", "")


def size_bytes(spec, values, sizefn=None):
    """the bytes the header's size function gives for this call's scalars (None: the parameter has none)"""
    if spec.size is None:
        return None
    fn, args, unit = spec.size
    a = tuple(int(x) for x in args(values))
    if callable(fn):
        return int(fn(*a)) * unit
    if sizefn is not None:
        return int(sizefn(fn, *a)) * unit
    from learning3d_amd import _lib
    f = getattr(_lib.lib(), fn)
    return int(f(*a)) * unit


def launch_grid_stats(name, *args):
    """`launch` for the undeclared entry point (as tests/test_gpu_chamfer_grid.py binds it)"""
    from learning3d_amd import _lib
    fn = getattr(_lib.lib(), GRID_STATS)
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 6
    raw = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    _lib.check(fn(*raw, torch.cuda.current_stream().cuda_stream), name)


class Arena:
    """the writable memory of one call: each tensor a slice of its own guarded buffer"""

    def __init__(self, fill, device="cuda", left=None):
        self.fill, self.device, self.left = fill, device, left
        self.slots = []                       # (raw uint8 buffer, offset, nbytes, tensor)

    def _slot(self, nbytes, key=None):
        if self.left is not None and key is not None:                       # the third run: the area the second run left behind
            for raw, off, n, t, k in self.left.slots:
                if k == key:
                    assert n == nbytes
                    self.slots.append((raw, off, n, t, k))
                    return raw[off:off + n], True
            raise KeyError(key)
        raw = torch.empty(GUARD + ALIGN + nbytes + GUARD, dtype=torch.uint8, device=self.device)
        off = GUARD + (-(raw.data_ptr() + GUARD)) % ALIGN
        raw.fill_(GUARD_BYTE)
        data = raw[off:off + nbytes]
        data.fill_(self.fill)
        assert nbytes == 0 or data.data_ptr() % ALIGN == 0
        self.slots.append([raw, off, nbytes, None, key])
        return data, False

    def out(self, dtype, *shape, key=None):
        """a writable tensor of exactly this size, holding the fill"""
        n = 1
        for s in shape:
            n *= int(s)
        data, reused = self._slot(n * torch.empty(0, dtype=dtype).element_size(), key)
        t = data.view(dtype).view(*[int(s) for s in shape])
        if not reused:
            self.slots[-1][3] = t
        return t

    def f32(self, *shape):
        return self.out(torch.float32, *shape)

    def bytes(self, nbytes, zero_first=0, key=None):
        """a workspace or an image: exactly nbytes bytes; zero_first: the header's "first n bytes zero before the first call" """
        t = self.out(torch.uint8, int(nbytes), key=key)
        if zero_first and not (self.left is not None and key is not None):
            t[:zero_first] = 0
        return t

    def inout(self, value, key=None):
        """a writable tensor prepared as the header's precondition says (the same under both fills)"""
        t = self.out(value.dtype, *value.shape, key=key)
        t.copy_(value)
        return t

    def slot_of(self, t):
        for raw, off, n, mine, _ in self.slots:
            if mine is not None and mine.data_ptr() == t.data_ptr() and n == t.numel() * t.element_size():
                return raw, off, n
        return None

    def guard_damage(self, t):
        """None, or the byte offset relative to t's first byte of the first damaged guard byte"""
        raw, off, n = self.slot_of(t)
        bad = raw != GUARD_BYTE
        bad[off:off + n] = False
        if not bool(bad.any()):
            return None
        return int(bad.nonzero()[0]) - off


def _bytes(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def _first_difference(a, b, open_ranges=()):
    d = _bytes(a) != _bytes(b)
    for lo, hi in open_ranges:
        d[max(lo, 0):hi] = False
    return int(d.nonzero()[0]) if bool(d.any()) else None


def _run(name, proto, build, launch, arena, contract, sizefn):
    args = list(build(arena))
    params = proto.params
    assert len(args) in (len(params), len(params) - 1), f"{name}: the case passes {len(args)} arguments, the header has {len(params)}"
    values = {p.name: a for p, a in zip(params, args)}
    consts, writable = [], []
    for p, a in zip(params, args):
        if not isinstance(a, torch.Tensor):
            continue
        if is_writable(p):
            assert arena.slot_of(a) is not None, f"{name}: the case did not take writable parameter `{p.name}` from the arena"
            spec = spec_of(name, p.name, contract)
            want = size_bytes(spec, values, sizefn)
            have = a.numel() * a.element_size()
            assert want is None or have == want, f"{name}: the case gives `{p.name}` {have} bytes, its size function says {want}"
            writable.append((p, a, spec))
        else:
            consts.append((p, a, a.clone()))
    launch(name, *args)
    if arena.device != "cpu":
        torch.cuda.synchronize()
    for p, a, _ in writable:
        at = arena.guard_damage(a)
        if at is not None:
            raise ContractError(f"{name}: parameter `{p.name}` ({a.numel() * a.element_size()} bytes): a guard byte was written at offset {at} "
                                f"of the tensor (fill {arena.fill:#04x})")
    for p, a, before in consts:
        at = _first_difference(a, before)
        if at is not None:
            raise ContractError(f"{name}: `const` parameter `{p.name}` was changed at byte offset {at}")
    return values, writable


def compare_runs(name, values, what1, w1, what2, w2):
    """(c) of the module text for two runs of one call: w1, w2 = [(parameter, tensor, spec)] of its writable tensors"""
    by_name = {pname: a for pname, a, _ in w2}
    count = by_name.get("count")
    for pname, a, spec in w1:
        if spec.kind == "scratch":
            continue
        b = by_name[pname]
        nbytes = a.numel() * a.element_size()
        if spec.open is None:
            open_ranges = []
        elif name == "l3d_mask_select":
            open_ranges = spec.open(values, nbytes, None if count is None else int(count.reshape(-1)[0]))
        else:
            open_ranges = spec.open(values, nbytes)
        if spec.bound is not None:
            assert spec.quote, f"{name}: a tolerance for `{pname}` must quote the header line that makes it order-dependent"
            bar = spec.bound(values)
            ok = (a.double() - b.double()).abs() <= bar          # (a NaN, an element never written under fill A, is not <= anything)
            if not bool(ok.all()):
                at = int((~ok).reshape(-1).nonzero()[0]) * a.element_size()
                raise ContractError(f"{name}: parameter `{pname}` differs beyond its summation bound at byte offset {at} of {nbytes} "
                                    f"between {what1} and {what2}")
            continue
        at = _first_difference(a, b, open_ranges)
        if at is not None:
            raise ContractError(f"{name}: parameter `{pname}` ({spec.kind}) differs at byte offset {at} of {nbytes} between {what1} and "
                                f"{what2}: an element that was not written, or a result that depends on what the memory held")


def check(name, build, launch=None, contract=None, proto=None, sizefn=None, device="cuda"):
    """Run entry point `name` with the arguments build(arena) under fill A and under fill B (and, where a workspace carries state from
    call to call, a third time on the workspace the second run left) and hold it to (a), (b), (c) of the module text.
    -> the writable tensors of the fill-B run, {parameter: tensor}: the values a case goes on to compare with its reference."""
    global ACTIVE
    if launch is None and DEFAULT_LAUNCH is not None:
        launch = DEFAULT_LAUNCH
    elif launch is None:
        from learning3d_amd import _lib
        launch = _lib.call
    proto = proto or prototypes()[name]
    ACTIVE, outer = (name, proto, contract, sizefn), ACTIVE
    try:
        return _check(name, build, launch, contract, proto, sizefn, device)
    finally:
        ACTIVE = outer


def _check(name, build, launch, contract, proto, sizefn, device):
    runs = []
    for label, fill in FILLS:
        arena = Arena(fill, device)
        runs.append((label, arena) + _run(name, proto, build, launch, arena, contract, sizefn))
    (_, arena_a, values, wa), (_, arena_b, _, wb) = runs
    compare = [("fill A (0xFF)", wa, "fill B (0x00)", wb)]
    if any(spec.keep for _, _, spec in wb):
        arena_c = Arena(FILL_A, device, left=arena_b)
        _, wc = _run(name, proto, build, launch, arena_c, contract, sizefn)
        compare.append(("a second call on the workspace the first left", wc, "the first call", wb))
    for what1, w1, what2, w2 in compare:
        compare_runs(name, values, what1, [(p.name, a, spec) for p, a, spec in w1], what2, [(p.name, a, spec) for p, a, spec in w2])
    if RECORD is not None:
        RECORD.append((name, values, {p.name: (a.clone(), spec) for p, a, spec in wb}))
    return {p.name: a for p, a, _ in wb}


# ------------------------------------------------------------------------------------------------------------------------------
# the same table under the public ops: an `inner` for layout_audit.install
def _overlap(a, b):
    sa, sb = a.untyped_storage(), b.untyped_storage()
    return sa.data_ptr() == sb.data_ptr()


def _fill_value(dtype, fill):
    if fill == FILL_B:
        return 0
    return float("nan") if dtype.is_floating_point else (255 if dtype == torch.uint8 else -1)


def filling_call(real_call, fill, log=None):
    """-> call(name, *args): before forwarding to real_call, fill every writable tensor argument with the fill (in-out parameters and
    the state bytes of a workspace are left as the wrapper prepared them; a tensor that shares its buffer with a const argument of the
    same call -- "y may alias x" -- is left too) and assert that each workspace / image is at least what its size function says."""
    def call(name, *args, **kw):
        proto = prototypes()[name]
        values = {p.name: a for p, a in zip(proto.params, args)}
        const_tensors = [a for p, a in zip(proto.params, args) if isinstance(a, torch.Tensor) and not is_writable(p)]
        for p, a in zip(proto.params, args):
            if not (isinstance(a, torch.Tensor) and is_writable(p)):
                continue
            spec = spec_of(name, p.name)
            want = size_bytes(spec, values)
            have = a.numel() * a.element_size()
            if want is not None and have < want:
                raise ContractError(f"{name}: the wrapper passes `{p.name}` {have} bytes; its size function says {want} for this call")
            inout = spec.kind == "inout" and (spec.inout_when is None or spec.inout_when(values))
            if inout or any(_overlap(a, c) for c in const_tensors):
                continue
            if log is not None:
                log.append((name, p.name))
            if spec.keep:
                flat = a.view(-1).view(torch.uint8)
                flat[spec.keep:].fill_(fill)
            else:
                a.fill_(_fill_value(a.dtype, fill))
        return real_call(name, *args, **kw)
    return call
