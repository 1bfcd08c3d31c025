"""DCP's pointer network (reference: utils/transformer.py:14-243).  Module / parameter names follow the
reference so its checkpoints load unchanged (model.encoder.layers.0.self_attn.linears.0.weight, ...
.norm.a_2, ...).  Without autograd, on the GPU and at tileable shapes the twelve Linear layers and the
two feed-forward blocks of a pass (62 % of its FLOPs) run on the bf16x3 1x1-conv kernel
(`l3d_pointwise_conv_split`: a Linear over points IS a 1x1 conv) with bias and ReLU folded into its
epilogue; its [B,Cout,N] output layout is consumed as is (heads become [B,h,d_k,N] views, the attention
matmuls take the transposes for free), the attention itself is one flash-style kernel
(`l3d_attention_forward`, no [B,h,N,N] score tensor) and LayerNorm one fused kernel (`l3d_layernorm_planes`)."""
import copy
import os
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .._lib import call, f32a, f32c, lib, on_device_of


FLASH_ATTENTION = True      # l3d_attention_forward for d_k in {32, 64, 128}; False: torch matmul + softmax + matmul
DEFER_LN_VALUES = True      # sublayer norms write only their fp16 plane image; fp32 values on demand (_ln_values)
PROJECTION_MAXIMA = True    # the f16x2 q|k|v projections report max|q|, |k|, |v| from their epilogues (False: a pass over q, k, v)
# autograd live (a training step, or the recompute behind a checkpointed forward): the nn.Linear layers and the attention core
# (q k^T, softmax, p v) on l3d_bmm_f32 / l3d_softmax_rows, forward and backward, the tensors read where they lie (models/_rows.py).
# "conv": the Linear layers through the channel-first conv / dgrad / wgrad kernels instead (two transposed copies per layer and
# direction: a DCP training step took 25.6 ms with it against 20.4 ms on rocBLAS, LABLOG R3.22 -- kept as a cross-check);
# "torch": nn.Linear and torch matmul / softmax (rocBLAS).  LayerNorm's HIP forward / backward is independent of this switch.
TRAIN_LINEAR = os.environ.get("L3D_TRAIN_LINEAR", "rows")
# the channel-first pass's plane images (LayerNorm outputs, attention contexts, the feed-forward's hidden layer) with an UNSCALED residual
# plane: every projection then runs the two-plane form of the f16x2 kernel (conv_f16.hip: 12 instead of 14 fragment reads, 4 instead
# of 5 DMA pieces per chunk); "0" keeps the scaled images of rounds 3-5 (A/B)
TWO_PLANE_IMAGES = os.environ.get("L3D_TWO_PLANE_IMAGES", "1") != "0"
CHANNEL_FIRST_PASS = True   # a whole encoder-decoder pass in the [B,C,N] layout the GEMMs write (Transformer._pass_cf); False: module by module

_ATT_WS = {}


def _attention_workspace(device, stream=None):
    """16 bytes per device AND stream for l3d_attention_forward_f16b's operand maxima (written and read on the launch stream: two
    streams sharing them would overwrite each other's).  stream: the raw stream handle, the device's current one by default."""
    if stream is None:
        stream = torch.cuda.current_stream(device).cuda_stream
    key = (str(device), stream)
    ws = _ATT_WS.get(key)
    if ws is None:
        ws = torch.zeros(4, dtype=torch.int32, device=device)
        _ATT_WS[key] = ws
    return ws


def _ln_values(t):
    """A LayerNorm output whose fp32 values were deferred (LayerNorm.forward(values=False): only the fp16 plane image was
    written): compute them now, into the tensor's own storage.  Everything in this module that READS such a tensor calls this
    first; the fast routes never do (they consume the image)."""
    pend = getattr(t, "_l3d_pending", None) if t is not None else None
    if pend is not None:
        xc, ln = pend
        C = xc.size(-1)
        call("l3d_layernorm_planes", xc, f32a(ln.a_2.detach()), f32a(ln.b_2.detach()), float(ln.eps), xc.numel() // C, C,
             t, None, tag="[values]")
        t._l3d_pending = None
    return t


def _planes_ok(fn):
    """Marks a sublayer callable whose every read of its input goes through _ln_values / the plane image."""
    fn._l3d_planes_ok = True
    return fn


def _fast_linear_ok(lin, x, n_points):
    """bf16x3 conv kernel applicable: inference, GPU, Cout % 256 == 0, points % 128 == 0, Cin % 16 == 0"""
    from ..models import _fused
    return (x.is_cuda and not (torch.is_grad_enabled() and (x.requires_grad or lin.weight.requires_grad))
            and _fused.split_eligible(lin.in_features, lin.out_features, n_points))


def _linear_cf(lin, x, channel_last, relu=False, out_scale=None, planes=None, out_planes=False, amax=None, residual=None,
               two_plane=False):
    """Linear over points as a 1x1 conv: x [B,N,Cin] (channel_last) or [B,Cin,N] -> [B,Cout,N];
    out_scale multiplies the whole result (weights and bias) in the kernel's epilogue.
    planes = (image, B, N): the input exists only as an fp16 plane image (x is None); out_planes: return (image, B, N) of the
    output instead of the fp32 tensor (f16x2 path only; None if that path does not apply).
    amax = (int32 tensor, channels per group): the f16x2 kernel also maximises max|y| per channel group into the tensor and
    the result carries `_l3d_amax = True`; ignored (no attribute) on the other routes.
    two_plane: the input image carries an UNSCALED residual plane (l3d_layernorm_planes_cf / l3d_attention_forward_f16b / a plane
    output of this route asked for one): the two-plane form of the f16x2 kernel; a plane output is unscaled as well."""
    from ..models import _fused
    if planes is not None:
        img, nb_, np_ = planes
    else:
        img = getattr(x, "_l3d_planes", None) if channel_last else None
        nb_, np_ = (x.size(0), x.size(1)) if img is not None else (0, 0)
    if img is not None and _fused.gemm_arith() == "f16x2" and _fused.f16_eligible(lin.in_features, lin.out_features, np_):
        # x is a LayerNorm output that came with its fp16 plane image: f16x2 kernel, no pass over x
        c16 = _fused.cached(lin.__dict__, "_l3d_split_f16", [lin.weight],
                            lambda: _fused.split_weights_f16(lin.weight.detach().float().contiguous()))
        bias = lin.bias.detach() if lin.bias is not None else None
        scale = None
        if out_scale is not None:
            scale = torch.full((lin.out_features,), float(out_scale), dtype=torch.float32, device=img.device)
            bias = bias * float(out_scale) if bias is not None else None
        if out_planes:
            return (_fused.pointwise_conv_f16(img, nb_, np_, c16, lin.in_features, lin.out_features, scale, bias, relu=relu,
                                              out_planes=True, unscaled=two_plane), nb_, np_)
        if amax is not None and amax[1] % 256 == 0 and PROJECTION_MAXIMA:
            y = _fused.pointwise_conv_f16(img, nb_, np_, c16, lin.in_features, lin.out_features, scale, bias, relu=relu, amax=amax,
                                          unscaled=two_plane)
            y._l3d_amax = True
            return y
        return _fused.pointwise_conv_f16(img, nb_, np_, c16, lin.in_features, lin.out_features, scale, bias, relu=relu,
                                         residual=residual, unscaled=two_plane)
    if out_planes:
        return None
    if residual is not None:
        raise RuntimeError("_linear_cf: the residual epilogue exists on the f16x2 plane route only")
    x = _ln_values(x)

    def split():
        w = lin.weight.detach().float().contiguous()
        return w, _fused.split_rows(w)
    w, ws = _fused.cached(lin.__dict__, "_l3d_split", [lin.weight], split)
    bias = lin.bias.detach() if lin.bias is not None else None
    scale = None
    if out_scale is not None:
        scale = torch.full((lin.out_features,), float(out_scale), dtype=torch.float32, device=x.device)
        bias = bias * float(out_scale) if bias is not None else None
    return _fused.pointwise_conv(x, w, scale, bias, relu=relu, channel_last=channel_last, w_split=ws)


def clones(module, N):
    return nn.ModuleList([copy.deepcopy(module) for _ in range(N)])


def attention(query, key, value, mask=None, dropout=None):
    d_k = query.size(-1)
    if mask is None and dropout is None and TRAIN_LINEAR == "rows" and query.is_cuda and query.dtype == torch.float32 \
            and key.size(-2) <= 8192 and query.shape[:-2] == key.shape[:-2] == value.shape[:-2] and 2 <= query.dim() <= 4 \
            and math.prod(query.shape[:-2]) <= 65535:         # what _rows / l3d_bmm_f32 take; anything else: the torch ops below
        from ..models import _rows
        return _rows.attention_core(query, key, value, 1.0 / math.sqrt(d_k))          # differentiable, HIP forward and backward
    scores = torch.matmul(query, key.transpose(-2, -1)) / math.sqrt(d_k)
    if mask is not None:
        scores = scores.masked_fill(mask == 0, -1e9)
    p_attn = F.softmax(scores, dim=-1)
    return torch.matmul(p_attn, value), p_attn


class LayerNorm(nn.Module):
    """reference :109-119 -- note: unbiased std and eps added to std, not nn.LayerNorm."""

    def __init__(self, features, eps=1e-6):
        super().__init__()
        self.a_2 = nn.Parameter(torch.ones(features))
        self.b_2 = nn.Parameter(torch.zeros(features))
        self.eps = eps

    def forward(self, x, values=True):
        """values=False (internal; SublayerConnection passes it for sublayers marked _planes_ok): when the output is also
        produced as an fp16 plane image, the fp32 values are not written until somebody asks (_ln_values)."""
        C = x.size(-1)
        if (x.is_cuda and x.dtype == torch.float32 and C % 4 == 0 and 1 < C <= 2048
                and not (torch.is_grad_enabled() and (x.requires_grad or self.a_2.requires_grad))):
            from ..models import _fused
            xc = f32a(x)                 # l3d_layernorm_planes reads whole rows 16 bytes at a time and refuses a misaligned x / a / b
            y = torch.empty_like(xc)
            rows = xc.numel() // C
            if (_fused.gemm_arith() == "f16x2" and x.dim() == 3 and C % 16 == 0 and C <= 512 and x.size(1) % 256 == 0):
                # also emit y as the fp16 plane image of the f16x2 conv kernel: the Linear layers that read this output
                # (_linear_cf) then need no split pass; the image rides on the tensor object
                img = torch.empty(lib().l3d_f16_image_bytes(1, rows, C), dtype=torch.uint8, device=xc.device)
                call("l3d_layernorm_planes", xc, f32a(self.a_2.detach()), f32a(self.b_2.detach()), float(self.eps), rows, C,
                     y if values else None, img)
                y._l3d_planes = img
                if not values:
                    y._l3d_pending = (xc, self)
                return y
            call("l3d_layernorm_planes", xc, f32a(self.a_2.detach()), f32a(self.b_2.detach()), float(self.eps), rows, C,
                 y, None, tag="[values]")
            return y
        if x.is_cuda:
            # autograd live (a training step, or the recompute of a checkpointed forward): HIP forward + one-pass HIP backward
            from ..models._train import layer_norm_ref
            return layer_norm_ref(x, self.a_2, self.b_2, self.eps)
        mean = x.mean(-1, keepdim=True)
        std = x.std(-1, keepdim=True)
        return self.a_2 * (x - mean) / (std + self.eps) + self.b_2


class SublayerConnection(nn.Module):
    def __init__(self, size, dropout=None):
        super().__init__()
        self.norm = LayerNorm(size)

    def forward(self, x, sublayer):
        # the fp32 values of the norm's output may be deferred only for sublayers that are known to read their input through
        # the plane image / _ln_values: the marked lambdas of this module, or a PositionwiseFeedForward whose forward is the
        # one defined here (not a subclass override) and that carries no hooks
        ok = getattr(sublayer, "_l3d_planes_ok", False)
        if ok and isinstance(sublayer, nn.Module):
            ok = (type(sublayer).forward is PositionwiseFeedForward.forward and not sublayer._forward_hooks
                  and not sublayer._forward_pre_hooks)
        if self.norm._forward_hooks or self.norm._forward_pre_hooks:
            ok = False
        y = sublayer(self.norm(x, values=not (DEFER_LN_VALUES and ok)))
        if (x.is_cuda and x.dim() == 3 and y.shape == x.shape and x.dtype == torch.float32 and y.dtype == torch.float32
                and x.is_contiguous() and not y.is_contiguous() and y.transpose(1, 2).is_contiguous()
                and not (torch.is_grad_enabled() and (x.requires_grad or y.requires_grad))):
            # the fast sublayers return a [B,N,C] VIEW of channel-first conv output: add through a tiled
            # transpose (l3d_add_transposed) instead of torch's strided elementwise kernel (3x slower)
            out = torch.empty_like(x)
            B, N, C = x.shape
            call("l3d_add_transposed", x, y.transpose(1, 2), B, N, C, out)
            return out
        return x + y


def _lin(lin, x, relu=False):
    """lin(x) (+ ReLU) where autograd is live (a training step, or the recompute behind a checkpointed forward): the GEMM, its
    dgrad and its wgrad on l3d_bmm_f32 over the rows as they lie (models/_rows.linear); TRAIN_LINEAR picks the other routes."""
    if x.is_cuda and torch.is_grad_enabled() and type(lin) is nn.Linear and x.numel() > 0 and x.dtype == torch.float32:
        if TRAIN_LINEAR == "rows":
            from ..models import _rows
            return _rows.linear(x, lin, relu=relu)
        if TRAIN_LINEAR == "conv" and lin.bias is not None:
            from ..models._train import hip_layers_ok, linear_act
            if hip_layers_ok(x):
                return linear_act(x, lin, relu=relu)
    y = lin(x)
    return F.relu(y) if relu else y


class MultiHeadedAttention(nn.Module):
    def __init__(self, h, d_model, dropout=0.1):
        super().__init__()
        assert d_model % h == 0
        self.d_k = d_model // h
        self.h = h
        self.linears = clones(nn.Linear(d_model, d_model), 4)
        self.attn = None
        self.dropout = None

    def _fused_linear(self, lo, hi):
        """nn.Linear whose weight / bias are linears[lo:hi] stacked (cached per parameter version): the
        projections of one input become a single 1x1-conv launch."""
        from ..models import _fused
        ps = [p for l in self.linears[lo:hi] for p in (l.weight, l.bias)]

        def build():
            lin = nn.Linear(self.linears[lo].in_features, sum(l.out_features for l in self.linears[lo:hi]),
                            device=self.linears[lo].weight.device)
            with torch.no_grad():
                lin.weight.copy_(torch.cat([l.weight for l in self.linears[lo:hi]], 0))
                lin.bias.copy_(torch.cat([l.bias for l in self.linears[lo:hi]], 0))
            lin.requires_grad_(False)
            return lin
        # a plain dict in the instance's __dict__, not a registered submodule: state_dict unchanged
        return _fused.cached(self.__dict__.setdefault("_l3d_fused", {}), (lo, hi), ps, build)

    def forward(self, query, key, value, mask=None):
        if mask is not None:
            mask = mask.unsqueeze(1)
        nb = query.size(0)
        if mask is None and all(_fast_linear_ok(self.linears[0], t, t.size(1)) for t in (query, key, value)):
            # channel-first projections: [B, h*d_k, N] viewed as [B, h, d_k, N] -- no head transposes
            C_ = self.h * self.d_k
            n_q, n_k = query.size(1), key.size(1)
            # projections that share an input run as ONE conv with concatenated weights (q|k|v for
            # self-attention, k|v for cross-attention); q, k, v are then channel slices of its [B, 3C, N] output
            # the f16x2 projections leave max|q|, |k|, |v| in the attention workspace from their own epilogues
            ws = _attention_workspace(query.device)
            ws.zero_()
            if query is key and key is value:
                qkv = _linear_cf(self._fused_linear(0, 3), query, True, amax=(ws, C_))
                q, k, v = qkv[:, :C_], qkv[:, C_:2 * C_], qkv[:, 2 * C_:]
                have_max = getattr(qkv, "_l3d_amax", False)
            elif key is value:
                q = _linear_cf(self.linears[0], query, True, amax=(ws, C_))
                kv = _linear_cf(self._fused_linear(1, 3), key, True, amax=(ws[1:], C_))
                k, v = kv[:, :C_], kv[:, C_:]
                have_max = getattr(q, "_l3d_amax", False) and getattr(kv, "_l3d_amax", False)
            else:
                q, k, v = [_linear_cf(lin, x, True, amax=(ws[i:], C_))
                           for i, (lin, x) in enumerate(zip(self.linears, (query, key, value)))]   # [B,C,N]
                have_max = all(getattr(z, "_l3d_amax", False) for z in (q, k, v))
            self.attn = None                                   # the [B,h,N,M] map is never formed
            if FLASH_ATTENTION and self.d_k in (32, 64, 128):
                from ..models import _fused
                out_lin = self.linears[-1]
                if (_fused.gemm_arith() == "f16x2" and C_ % 16 == 0
                        and _fused.f16_eligible(out_lin.in_features, out_lin.out_features, n_q)):
                    # both GEMMs as f16x2 (operand scales from the tensors' maxima); the context leaves the kernel as the
                    # fp16 plane image of the f16x2 conv kernel, so the output projection needs no split pass either
                    img = torch.empty(lib().l3d_f16_image_bytes(1, nb * n_q, C_), dtype=torch.uint8, device=q.device)
                    call("l3d_attention_forward_f16b", q, k, v, nb, self.h, self.d_k, n_q, n_k, q.stride(0), k.stride(0), v.stride(0),
                         1.0 / math.sqrt(self.d_k), ws, int(bool(have_max)), None, img)
                    return _linear_cf(out_lin, None, True, planes=(img, nb, n_q)).transpose(1, 2)     # [B,N,C] view
                ctx = torch.empty((nb, C_, n_q), dtype=torch.float32, device=q.device)
                if _fused.gemm_arith() == "f16x2":
                    call("l3d_attention_forward_f16b", q, k, v, nb, self.h, self.d_k, n_q, n_k, q.stride(0), k.stride(0), v.stride(0),
                         1.0 / math.sqrt(self.d_k), ws, int(bool(have_max)), ctx, None)
                else:
                    call("l3d_attention_forward_strided", q, k, v, nb, self.h, self.d_k, n_q, n_k, q.stride(0), k.stride(0), v.stride(0),
                         1.0 / math.sqrt(self.d_k), ctx)
            else:
                qh, kh, vh = [z.reshape(nb, self.h, self.d_k, z.size(2)) for z in (q, k, v)]
                p = F.softmax(torch.matmul(qh.transpose(-2, -1), kh) / math.sqrt(self.d_k), dim=-1)   # [B,h,N,M]
                ctx = torch.matmul(vh, p.transpose(-2, -1)).reshape(nb, C_, n_q)
            return _linear_cf(self.linears[-1], ctx, False).transpose(1, 2)                       # [B,N,C] view
        q, k, v = [_lin(lin, _ln_values(x)).view(nb, -1, self.h, self.d_k).transpose(1, 2)
                   for lin, x in zip(self.linears, (query, key, value))]
        x, self.attn = attention(q, k, v, mask=mask, dropout=self.dropout)
        x = x.transpose(1, 2).contiguous().view(nb, -1, self.h * self.d_k)
        return _lin(self.linears[-1], x)


class PositionwiseFeedForward(nn.Module):
    _l3d_planes_ok = True          # reads its input through the plane image or _ln_values only

    def __init__(self, d_model, d_ff, dropout=0.1):
        super().__init__()
        self.w_1 = nn.Linear(d_model, d_ff)
        self.norm = nn.Sequential()
        self.w_2 = nn.Linear(d_ff, d_model)
        self.dropout = None

    def forward(self, x):
        if x.dim() == 3 and _fast_linear_ok(self.w_1, x, x.size(1)) and _fast_linear_ok(self.w_2, x, x.size(1)):
            from ..models import _fused
            if _fused.gemm_arith() == "f16x2" and _fused.f16_eligible(self.w_2.in_features, self.w_2.out_features, x.size(1)):
                hp = _linear_cf(self.w_1, x, True, relu=True, out_planes=True)      # hidden layer as fp16 planes, never fp32
                if hp is not None:
                    return _linear_cf(self.w_2, None, True, planes=hp).transpose(1, 2)
            h = _linear_cf(self.w_1, x, True, relu=True)                  # [B,d_ff,N]
            return _linear_cf(self.w_2, h, False).transpose(1, 2)         # [B,N,d_model] view
        return _lin(self.w_2, _lin(self.w_1, _ln_values(x), relu=True))


class EncoderLayer(nn.Module):
    def __init__(self, size, self_attn, feed_forward, dropout):
        super().__init__()
        self.self_attn = self_attn
        self.feed_forward = feed_forward
        self.sublayer = clones(SublayerConnection(size, dropout), 2)
        self.size = size

    def forward(self, x, mask):
        x = self.sublayer[0](x, _planes_ok(lambda y: self.self_attn(y, y, y, mask)))
        return self.sublayer[1](x, self.feed_forward)


class DecoderLayer(nn.Module):
    def __init__(self, size, self_attn, src_attn, feed_forward, dropout):
        super().__init__()
        self.size = size
        self.self_attn = self_attn
        self.src_attn = src_attn
        self.feed_forward = feed_forward
        self.sublayer = clones(SublayerConnection(size, dropout), 3)

    def forward(self, x, memory, src_mask, tgt_mask):
        x = self.sublayer[0](x, _planes_ok(lambda y: self.self_attn(y, y, y, tgt_mask)))
        x = self.sublayer[1](x, _planes_ok(lambda y: self.src_attn(y, memory, memory, src_mask)))
        return self.sublayer[2](x, self.feed_forward)


class Encoder(nn.Module):
    def __init__(self, layer, N):
        super().__init__()
        self.layers = clones(layer, N)
        self.norm = LayerNorm(layer.size)

    def forward(self, x, mask):
        for layer in self.layers:
            x = layer(x, mask)
        return self.norm(x)


class Decoder(nn.Module):
    def __init__(self, layer, N):
        super().__init__()
        self.layers = clones(layer, N)
        self.norm = LayerNorm(layer.size)

    def forward(self, x, memory, src_mask, tgt_mask):
        for layer in self.layers:
            x = layer(x, memory, src_mask, tgt_mask)
        return self.norm(x)


class EncoderDecoder(nn.Module):
    def __init__(self, encoder, decoder, src_embed, tgt_embed, generator):
        super().__init__()
        self.encoder = encoder
        self.decoder = decoder
        self.src_embed = src_embed
        self.tgt_embed = tgt_embed
        self.generator = generator

    def forward(self, src, tgt, src_mask, tgt_mask):
        memory = self.encoder(self.src_embed(src), src_mask)
        return self.generator(self.decoder(self.tgt_embed(tgt), memory, src_mask, tgt_mask))


class Identity(nn.Module):
    def forward(self, *input):
        return input


class Transformer(nn.Module):
    """reference :219-243.  forward(src [B,C,N], tgt [B,C,N]) -> (src_embedding, tgt_embedding)."""
    _l3d_train_direct = True       # _fused.checkpointed: in train() mode the forward runs once, on the differentiable routes

    def __init__(self, emb_dims, n_blocks, dropout, ff_dims, n_heads):
        super().__init__()
        self.emb_dims, self.N, self.dropout = emb_dims, n_blocks, dropout
        self.ff_dims, self.n_heads = ff_dims, n_heads
        c = copy.deepcopy
        attn = MultiHeadedAttention(n_heads, emb_dims)
        ff = PositionwiseFeedForward(emb_dims, ff_dims, dropout)
        self.model = EncoderDecoder(Encoder(EncoderLayer(emb_dims, c(attn), c(ff), dropout), n_blocks),
                                    Decoder(DecoderLayer(emb_dims, c(attn), c(attn), c(ff), dropout), n_blocks),
                                    nn.Sequential(), nn.Sequential(), nn.Sequential())

    def forward(self, *input):
        """The fused pointer network serves the forward of an eval() module in every grad mode (dropout is None throughout, reference
        :163-217); a backward recomputes through the reference's op sequence (_fused.checkpointed).  A train() module with something
        to learn runs the forward once, under autograd, on the differentiable routes (_l3d_train_direct)."""
        from ..models import _fused
        return _fused.checkpointed(self, self._forward, input[0], input[1])

    # ------------------------------------------------------------------------------------------------------------------
    # One encoder-decoder pass with every tensor in the layout the GEMMs write, [B,C,N]: LayerNorm over the channels of a
    # channel-first tensor straight to the fp16 plane image (l3d_layernorm_planes_cf), q|k|v / q, k|v projections with their
    # maxima, attention with its context as planes, output projection and the feed-forward's second layer with the
    # sublayer's residual connection in their epilogues (l3d_pointwise_conv_f16 with a residual).  Against the module-by-module
    # route this drops, per pass, five transposed residual adds, the .contiguous() copies around the pass and the fp32
    # LayerNorm outputs nobody reads (reference: utils/transformer.py:131-140 SublayerConnection, :163-217, :236-243).
    # ------------------------------------------------------------------------------------------------------------------
    def _cf_pass_ok(self, src, tgt):
        from ..models import _fused
        C = self.emb_dims
        if not (CHANNEL_FIRST_PASS and FLASH_ATTENTION and PROJECTION_MAXIMA and _fused.gemm_arith() == "f16x2"):
            return False
        if not (src.is_cuda and tgt.is_cuda and src.dtype == torch.float32 and tgt.dtype == torch.float32 and src.dim() == 3
                and tgt.dim() == 3 and src.size(1) == C and tgt.size(1) == C and src.size(0) == tgt.size(0)):
            return False
        if C not in (256, 512) or self.ff_dims % 256 or src.size(2) % 256 or tgt.size(2) % 256 or C // self.n_heads not in (32, 64, 128):
            return False
        if torch.is_grad_enabled() and (src.requires_grad or tgt.requires_grad or any(p.requires_grad for p in self.parameters())):
            return False
        m = self.model
        if any(len(e) for e in (m.src_embed, m.tgt_embed, m.generator)):
            return False
        stock = {EncoderDecoder, Encoder, Decoder, EncoderLayer, DecoderLayer, SublayerConnection, LayerNorm, MultiHeadedAttention,
                 PositionwiseFeedForward, nn.Linear, nn.Sequential, nn.ModuleList}
        for mod in m.modules():                    # subclasses, overrides and hooks see the module-by-module route
            if type(mod) not in stock or mod._forward_hooks or mod._forward_pre_hooks:
                return False
        return all(_fused.f16_eligible(a, b, n) for a, b, n in ((C, C, src.size(2)), (C, C, tgt.size(2)), (C, self.ff_dims, src.size(2)),
                                                               (self.ff_dims, C, tgt.size(2))))

    @staticmethod
    def _ln_cf(norm, x, values=False, planes=True):
        """LayerNorm over the channels of x [B,C,N] -> (fp32 [B,C,N] or None, plane image or None)"""
        B, C, N = x.shape
        y = torch.empty_like(x) if values else None
        img = torch.empty(lib().l3d_f16_image_bytes(1, B * N, C), dtype=torch.uint8, device=x.device) if planes else None
        call("l3d_layernorm_planes_cf", x, norm.a_2.detach().contiguous(), norm.b_2.detach().contiguous(), float(norm.eps), B, C, N,
             y, img, int(TWO_PLANE_IMAGES))
        return y, img

    def _attn_block_cf(self, norm, attn, x, memory):
        """x + attn(norm(x), m, m) with m = norm(x) (self-attention, memory None) or the encoder's output image (memory = (img, N_m))"""
        B, C, N = x.shape
        _, img = self._ln_cf(norm, x)
        ws = _attention_workspace(x.device)
        ws.zero_()
        if memory is None:
            qkv = _linear_cf(attn._fused_linear(0, 3), None, True, planes=(img, B, N), amax=(ws, C), two_plane=TWO_PLANE_IMAGES)
            q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
            have_max, M = getattr(qkv, "_l3d_amax", False), N
        else:
            mem_img, M = memory
            q = _linear_cf(attn.linears[0], None, True, planes=(img, B, N), amax=(ws, C), two_plane=TWO_PLANE_IMAGES)
            kv = _linear_cf(attn._fused_linear(1, 3), None, True, planes=(mem_img, B, M), amax=(ws[1:], C), two_plane=TWO_PLANE_IMAGES)
            k, v = kv[:, :C], kv[:, C:]
            have_max = getattr(q, "_l3d_amax", False) and getattr(kv, "_l3d_amax", False)
        attn.attn = None                                           # the [B,h,N,M] map is never formed
        ctx = torch.empty(lib().l3d_f16_image_bytes(1, B * N, C), dtype=torch.uint8, device=x.device)
        call("l3d_attention_forward_f16b", q, k, v, B, attn.h, attn.d_k, N, M, q.stride(0), k.stride(0), v.stride(0),
             1.0 / math.sqrt(attn.d_k), ws, int(bool(have_max)) | (2 if TWO_PLANE_IMAGES else 0), None, ctx)
        return _linear_cf(attn.linears[-1], None, True, planes=(ctx, B, N), residual=x, two_plane=TWO_PLANE_IMAGES)

    def _ffn_block_cf(self, norm, ff, x):
        B, C, N = x.shape
        _, img = self._ln_cf(norm, x)
        hidden = _linear_cf(ff.w_1, None, True, planes=(img, B, N), relu=True, out_planes=True, two_plane=TWO_PLANE_IMAGES)   # fp16 planes, never fp32
        return _linear_cf(ff.w_2, None, True, planes=hidden, residual=x, two_plane=TWO_PLANE_IMAGES)

    def _pass_cf(self, src, tgt):
        """self.model(src^T, tgt^T, None, None)^T for channel-first src, tgt [B,C,N]: the decoder's output [B,C,N_tgt]"""
        enc, dec = self.model.encoder, self.model.decoder
        x = f32c(src)
        for layer in enc.layers:
            x = self._attn_block_cf(layer.sublayer[0].norm, layer.self_attn, x, None)
            x = self._ffn_block_cf(layer.sublayer[1].norm, layer.feed_forward, x)
        _, mem = self._ln_cf(enc.norm, x)                          # the memory is only ever read by the k|v projections
        y = f32c(tgt)
        for layer in dec.layers:
            y = self._attn_block_cf(layer.sublayer[0].norm, layer.self_attn, y, None)
            y = self._attn_block_cf(layer.sublayer[1].norm, layer.src_attn, y, (mem, x.size(2)))
            y = self._ffn_block_cf(layer.sublayer[2].norm, layer.feed_forward, y)
        return self._ln_cf(dec.norm, y, values=True, planes=False)[0]

    def _forward(self, *input):
        if self._cf_pass_ok(input[0], input[1]):
            with on_device_of(input[0], input[1]):
                tgt_embedding = self._pass_cf(input[0], input[1])
                src_embedding = self._pass_cf(input[1], input[0])
            return src_embedding, tgt_embedding
        src = input[0].transpose(2, 1).contiguous()
        tgt = input[1].transpose(2, 1).contiguous()
        tgt_embedding = self.model(src, tgt, None, None).transpose(2, 1).contiguous()
        src_embedding = self.model(tgt, src, None, None).transpose(2, 1).contiguous()
        return src_embedding, tgt_embedding
