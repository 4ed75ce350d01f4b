"""decoders.py — host-side mirror of the reference's models/implicit_net.py for the MI355X path.

Same public names, constructor signatures, forward signatures and state-dict keys
(`linear_{1..4}.{weight,bias}`, `offset_enc.{weight,bias}`) as the reference
(models/implicit_net.py:42-57 get_embedder, :60-98 IMNet, :100-152 IEF), so checkpoints restore
with the reference's `restore()` (utils/training_utils.py:27-63) and the modules drop into
`LIDF.build_model` (models/pipeline.py:69-85).

Execution:
  * CUDA f32 input, no autograd needed  -> liblidf_hip.so (hand-written gfx950 kernels);
  * autograd needed (training)          -> liblidf_hip.so as well: a forward that keeps the
    activations (lidf_decoder_forward_train_f32) and a backward (lidf_decoder_backward_f32)
    behind a torch.autograd.Function; `forward_composite` is the same function written in
    torch ops, kept as the differentiable definition the tests compare against;
  * CPU input                           -> RuntimeError. There is no CPU product path.
"""
import ctypes as C

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib

# SURVEY 8b asked the drop-in modules to fall back to composite PyTorch where the HIP op does not apply.
# The product path has no CPU fallback — a CPU tensor raises, as the reference's CHECK_CUDA does — because
# a silent fallback would let "GPU" results come from torch ops. For checkpoint conversion or unit tests of
# code that merely CALLS the modules on the CPU, LIDF_ALLOW_CPU_COMPOSITE=1 routes CPU tensors (only those)
# through forward_composite — the same function in plain torch ops, never the oracle, never a CUDA tensor.
_CPU_HINT = "set LIDF_ALLOW_CPU_COMPOSITE=1 to run CPU tensors through the torch-op definition"


def _cpu_composite_allowed():
    import os
    return os.environ.get("LIDF_ALLOW_CPU_COMPOSITE") == "1"




# --------------------------------------------------------------------------------------------
# Positional encoding
# --------------------------------------------------------------------------------------------
class _EmbedFn(torch.autograd.Function):
    """embed(x) with the HIP backward lidf_embed_backward_f32."""

    @staticmethod
    def forward(ctx, x2, multires):
        x = x2.detach().contiguous()
        out = torch.empty((x.shape[0], 3 + 6 * multires), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().lidf_embed_f32(_lib.ptr(x), x.shape[0], multires, _lib.ptr(out),
                                                 _lib.current_stream(x.device)))
        ctx.save_for_backward(x)
        ctx.multires = multires
        return out

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        g = g.detach().contiguous().float()
        dx = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().lidf_embed_backward_f32(_lib.ptr(x), _lib.ptr(g), x.shape[0], ctx.multires,
                                                          _lib.ptr(dx), _lib.current_stream(x.device)))
        return dx, None


class Embedder:
    """Counterpart of the reference Embedder (models/implicit_net.py:9-39) for the one
    configuration get_embedder builds: include_input, log-sampled 2^0..2^(L-1), [sin, cos]."""

    def __init__(self, multires, input_dims=3):
        if input_dims != 3:
            raise ValueError("lidf_hip embedder supports input_dims == 3")
        self.multires = int(multires)
        self.out_dim = 3 + 6 * self.multires

    def embed(self, inputs):
        if not inputs.is_cuda:
            raise RuntimeError("embed: inputs must be a CUDA tensor (no CPU path)")
        if inputs.dtype != torch.float32:
            raise RuntimeError("embed: float32 required")
        if inputs.shape[-1] != 3:
            raise RuntimeError("embed: last dim must be 3")
        lead = inputs.shape[:-1]
        if torch.is_grad_enabled() and inputs.requires_grad:
            return _EmbedFn.apply(inputs.reshape(-1, 3), self.multires).reshape(*lead, self.out_dim)
        x = inputs.detach()
        x2 = x.reshape(-1, 3).contiguous()
        out = torch.empty((x2.shape[0], self.out_dim), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().lidf_embed_f32(_lib.ptr(x2), x2.shape[0], self.multires,
                                                 _lib.ptr(out), _lib.current_stream(x.device)))
        return out.reshape(*lead, self.out_dim)

    def embed_composite(self, inputs):
        """The same function in differentiable torch ops (the definition the tests compare with)."""
        outs = [inputs]
        for o in range(self.multires):
            f = float(2 ** o)
            outs.append(torch.sin(inputs * f))
            outs.append(torch.cos(inputs * f))
        return torch.cat(outs, -1)


def get_embedder(multires, i=0):
    """models/implicit_net.py:42-57 — returns (embed_fn, out_dim)."""
    if i == -1:
        return nn.Identity(), 3
    embedder_obj = Embedder(multires)
    embed = lambda x, eo=embedder_obj: eo.embed(x)  # noqa: E731
    return embed, embedder_obj.out_dim


# --------------------------------------------------------------------------------------------
# Decoders
# --------------------------------------------------------------------------------------------
def _leaky_clamp(y):
    return torch.max(torch.min(y, y * 0.01 + 0.99), y * 0.01)


def _init_offset_value(mod):
    """IEF.init_offset (implicit_net.py:104) as a Python float, read from the device once."""
    v = mod.__dict__.get("_init_offset_f")
    if v is None:
        io = mod.init_offset
        v = float(io.reshape(-1)[0].item()) if torch.is_tensor(io) else float(io)
        mod.__dict__["_init_offset_f"] = v
    return v


_LAYERS = ("linear_1", "linear_2", "linear_3", "linear_4", "offset_enc")


def decoder_params(mod):
    """The parameters of an IMNet / IEF in the order of LidfDecoder's pointer fields (w1, b1, ..., w4, b4, then
    an IEF's wenc, benc): the order every training node passes and returns them in."""
    return [t for name in _LAYERS if hasattr(mod, name) for t in (getattr(mod, name).weight, getattr(mod, name).bias)]


def n_passes(mod):
    """Passes of the trunk per row: an IEF's n_iter, 1 for an IMNet."""
    return int(mod.n_iter) if isinstance(mod, IEF) else 1


def _decoder_struct(mod, keep, tensors=None):
    """Fill a LidfDecoder from a module's parameters; `keep` collects the contiguous tensors
    whose storage the struct borrows for the duration of the call. `tensors` (in decoder_params
    order) overrides the module's live parameters: autograd's backward passes what its forward
    saved, so that an in-place update between the two is caught by torch's version check.
    An IMNet leaves wenc / benc NULL."""
    d = _lib.LidfDecoder()
    for (field, _), t in zip(d._fields_, decoder_params(mod) if tensors is None else tensors):
        setattr(d, field, _lib.param_ptr(t, keep))
    is_ief = isinstance(mod, IEF)
    d.n_iter = n_passes(mod)
    d.init_offset = _init_offset_value(mod) if is_ief else 0.0
    d.is_ief = 1 if is_ief else 0
    d.use_sigmoid = 1 if mod.use_sigmoid else 0
    return d


def _grad_struct(params):
    """Fresh float32 gradients shaped like `params` (decoder_params order) and the LidfDecoderGrads that points
    at them; an IMNet's wenc / benc stay NULL."""
    grads = [torch.empty(p.shape, dtype=torch.float32, device=p.device) for p in params]
    gs = _lib.LidfDecoderGrads()
    for (field, _), g in zip(gs._fields_, grads):
        setattr(gs, field, g.data_ptr())
    return grads, gs


def _rows(inp_feat):
    """[n, D] rows as the kernels read them: unit column stride, row stride >= D (a copy otherwise); returns the
    rows and their leading dimension."""
    x = inp_feat.detach()
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    n, d = x.shape
    return x, (x.stride(0) if n > 1 else d)


def is_shipped(mod):
    """The widths the register-chained kernels are built for (every shipped config): gf_dim 64, out_dim 1."""
    return mod.gf_dim == 64 and mod.linear_4.out_features == 1


def _check_supported(mod, what="this entry"):
    """Entries without a layer-by-layer counterpart (training, the fused query, stage 2). (The frame call takes gf_dim
    32 / 64 / 128 and states its own refusals: pipeline.FrameRunner.)"""
    if not is_shipped(mod):
        raise RuntimeError("lidf_hip: %s is built for gf_dim=64, out_dim=1 (every shipped config); got "
                           "gf_dim=%d out_dim=%d. Inference at other widths runs layer by layer "
                           "(IMNet / IEF forward without autograd, generic.decoder_forward)"
                           % (what, mod.gf_dim, mod.linear_4.out_features))


def decoders_forward(inp_feat, prob_dec=None, offset_dec=None, precision="f32"):
    """Run one or both decoders on a materialised [n, D] input through liblidf_hip
    (lidf_decoders_f32; precision="f16x3": lidf_decoders_split_f32, the split-f16 products of
    lidf_query; decoders of gf_dim 32 / 128: lidf_decoder_chain_split_f32). Returns (pred_prob or None, pred_offset or None), each [n,1]."""
    if precision not in ("f32", "f16x3"):
        raise ValueError("precision must be 'f32' or 'f16x3'")
    if prob_dec is None and offset_dec is None:
        raise ValueError("need at least one decoder")
    if not inp_feat.is_cuda:
        raise RuntimeError("inp_feat must be a CUDA tensor (no CPU path)")
    if inp_feat.dtype != torch.float32 or inp_feat.dim() != 2:
        raise RuntimeError("inp_feat must be float32 [n, D]")
    x, ld = _rows(inp_feat)
    n, d = x.shape
    keep = []
    dp = do = None
    for m in (prob_dec, offset_dec):
        if m is not None and m.inp_dim != d:
            raise RuntimeError("decoder inp_dim %d != input width %d" % (m.inp_dim, d))
    if any(m is not None and not is_shipped(m) for m in (prob_dec, offset_dec)):
        # widths other than the shipped ones: generic.py — the one-launch chain (either precision) or layer by layer
        # (f32 only; generic.split_refusal states why)
        from . import generic
        return (generic.decoder_forward(prob_dec, x, precision) if prob_dec is not None else None,
                generic.decoder_forward(offset_dec, x, precision) if offset_dec is not None else None)
    if prob_dec is not None:
        dp = _decoder_struct(prob_dec, keep)
    if offset_dec is not None:
        do = _decoder_struct(offset_dec, keep)
    out_p = torch.empty((n, 1), dtype=torch.float32, device=x.device) if dp is not None else None
    out_o = torch.empty((n, 1), dtype=torch.float32, device=x.device) if do is not None else None
    L = _lib.lib()
    wsb = L.lidf_decoders_workspace_bytes(n, d)
    ws = _lib.workspace(wsb, x.device)
    with torch.cuda.device(x.device):
        fn = L.lidf_decoders_split_f32 if precision == "f16x3" else L.lidf_decoders_f32
        _lib.check(fn(
            _lib.ptr(x), n, d, ld,
            C.byref(dp) if dp is not None else None, C.byref(do) if do is not None else None,
            _lib.ptr(out_p), _lib.ptr(out_o), _lib.ptr(ws), wsb, _lib.current_stream(x.device)))
    return out_p, out_o


class _DecoderTrainFn(torch.autograd.Function):
    """IMNet / IEF on [n, D] rows with a HIP forward that keeps the activations and a HIP backward
    (what autograd derives for models/implicit_net.py:81-98 / :131-152)."""

    @staticmethod
    def forward(ctx, mod, inp_feat, *params):
        x, ld = _rows(inp_feat)
        n, d = x.shape
        keep = []
        dec = _decoder_struct(mod, keep)
        L = _lib.lib()
        f32 = dict(dtype=torch.float32, device=x.device)
        act = torch.empty((max(L.lidf_decoder_train_act_floats(n, n_passes(mod)), 1),), **f32)
        wsb = L.lidf_decoder_train_workspace_bytes(n, d)
        ws = _lib.workspace(wsb, x.device)
        out = torch.empty((n, 1), **f32)
        with torch.cuda.device(x.device):
            _lib.check(L.lidf_decoder_forward_train_f32(
                _lib.ptr(x), n, d, ld, C.byref(dec), _lib.ptr(out), _lib.ptr(act), _lib.ptr(ws), wsb,
                _lib.current_stream(x.device)))
        # the parameters are saved (not re-read from the module in backward): torch's version
        # counters then catch an in-place update between forward and backward
        ctx.mod, ctx.ld, ctx.ws, ctx.wsb = mod, ld, ws, wsb
        ctx.save_for_backward(x, act, *params)
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, act, *params = ctx.saved_tensors
        n, d = x.shape
        keep = []
        dec = _decoder_struct(ctx.mod, keep, params)
        f32 = dict(dtype=torch.float32, device=x.device)
        g = g_out.detach().reshape(-1).contiguous().float()
        grads, gs = _grad_struct(params)
        d_inp = torch.empty((n, d), **f32) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().lidf_decoder_backward_f32(
                _lib.ptr(x), n, d, ctx.ld, C.byref(dec), _lib.ptr(act), _lib.ptr(g),
                _lib.ptr(d_inp), d, C.byref(gs), _lib.ptr(ctx.ws), ctx.wsb,
                _lib.current_stream(x.device)))
        # frozen parameters get no gradient tensor
        return (None, d_inp) + tuple(gr if ctx.needs_input_grad[2 + i] else None for i, gr in enumerate(grads))


class _DecoderPairTrainFn(torch.autograd.Function):
    """prob_dec(inp), offset_dec(inp) (models/pipeline.py:434-435) as ONE autograd node: the two forwards of
    _DecoderTrainFn, and a backward whose rows' gradient is one K = 512 product over both decoders' summed dZ1,
    stored once (lidf_decoder_pair_backward_f32) — two nodes run two K = 256 products, store [n, D] twice and
    leave the sum to autograd's accumulation launch."""

    @staticmethod
    def forward(ctx, prob, off, inp_feat, n_prob, *params):
        x, ld = _rows(inp_feat)
        n, d = x.shape
        keep = []
        L = _lib.lib()
        f32 = dict(dtype=torch.float32, device=x.device)
        wsb = L.lidf_decoder_pair_workspace_bytes(n, d)
        one = L.lidf_decoder_train_workspace_bytes(n, d)
        ws = _lib.workspace(wsb, x.device)
        outs, acts = [], []
        with torch.cuda.device(x.device):
            for which, mod in enumerate((prob, off)):
                dec = _decoder_struct(mod, keep)
                act = torch.empty((max(L.lidf_decoder_train_act_floats(n, n_passes(mod)), 1),), **f32)
                out = torch.empty((n, 1), **f32)
                _lib.check(L.lidf_decoder_forward_train_f32(
                    _lib.ptr(x), n, d, ld, C.byref(dec), _lib.ptr(out), _lib.ptr(act),
                    ws.data_ptr() + L.lidf_decoder_pair_workspace_offset(n, d, which), one,
                    _lib.current_stream(x.device)))
                outs.append(out)
                acts.append(act)
        ctx.prob, ctx.off, ctx.ld, ctx.ws, ctx.wsb, ctx.n_prob = prob, off, ld, ws, wsb, n_prob
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, acts[0], acts[1], *params)
        return outs[0], outs[1]

    @staticmethod
    def backward(ctx, g_p, g_o):
        x, act_p, act_o, *params = ctx.saved_tensors
        params_p, params_o = params[:ctx.n_prob], params[ctx.n_prob:]
        n, d = x.shape
        keep = []
        f32 = dict(dtype=torch.float32, device=x.device)
        # an output the loss did not use: a zero gradient (every sum of that decoder's backward is then zero)
        g_p = torch.zeros((n,), **f32) if g_p is None else g_p.detach().reshape(-1).contiguous().float()
        g_o = torch.zeros((n,), **f32) if g_o is None else g_o.detach().reshape(-1).contiguous().float()
        dp = _decoder_struct(ctx.prob, keep, params_p)
        do = _decoder_struct(ctx.off, keep, params_o)
        gt_p, gs_p = _grad_struct(params_p)
        gt_o, gs_o = _grad_struct(params_o)
        d_inp = torch.empty((n, d), **f32) if ctx.needs_input_grad[2] else None
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().lidf_decoder_pair_backward_f32(
                _lib.ptr(x), n, d, ctx.ld, C.byref(dp), C.byref(do), _lib.ptr(act_p), _lib.ptr(act_o),
                _lib.ptr(g_p), _lib.ptr(g_o), _lib.ptr(d_inp), d, C.byref(gs_p), C.byref(gs_o),
                _lib.ptr(ctx.ws), ctx.wsb, _lib.current_stream(x.device)))
        return (None, None, d_inp, None) + tuple(g if ctx.needs_input_grad[4 + i] else None
                                                 for i, g in enumerate(gt_p + gt_o))


def decoders_forward_train(inp_feat, prob_dec, offset_dec):
    """(prob_dec(inp_feat), offset_dec(inp_feat)) under autograd as one node — the two lines of LIDF.get_pred
    (models/pipeline.py:434-435) in one call. Same values and gradients as calling the two modules (the rows'
    gradient is one product over both decoders instead of two products and an accumulation). Shipped widths;
    other widths fall back to the modules' own calls."""
    if not is_shipped(prob_dec) or not is_shipped(offset_dec):
        return prob_dec(inp_feat), offset_dec(inp_feat)
    if not inp_feat.is_cuda:
        raise RuntimeError("decoders_forward_train: CUDA tensor required (no CPU path; " + _CPU_HINT + ")")
    for m in (prob_dec, offset_dec):
        if inp_feat.dtype != torch.float32 or inp_feat.dim() != 2 or inp_feat.shape[1] != m.inp_dim:
            raise RuntimeError("inp_feat must be float32 [n, %d]" % m.inp_dim)
    if not (prob_dec._needs_autograd(inp_feat) or offset_dec._needs_autograd(inp_feat)):
        return decoders_forward(inp_feat, prob_dec, offset_dec)     # nothing to differentiate: the inference launch
    pp, po = decoder_params(prob_dec), decoder_params(offset_dec)
    return _DecoderPairTrainFn.apply(prob_dec, offset_dec, inp_feat, len(pp), *pp, *po)


class _DecoderBase(nn.Module):
    def _forward_train(self, inp_feat):
        """Differentiable forward through liblidf_hip (training)."""
        if not is_shipped(self):   # other widths: every layer its own autograd function (generic.py)
            if not inp_feat.is_cuda or inp_feat.dtype != torch.float32 or inp_feat.dim() != 2:
                raise RuntimeError("inp_feat must be a CUDA float32 [n, %d]" % self.inp_dim)
            from . import generic
            return generic.decoder_forward_train(self, inp_feat)
        if inp_feat.dtype != torch.float32 or inp_feat.dim() != 2 or inp_feat.shape[1] != self.inp_dim:
            raise RuntimeError("inp_feat must be float32 [n, %d]" % self.inp_dim)
        return _DecoderTrainFn.apply(self, inp_feat, *decoder_params(self))

    def _needs_autograd(self, inp_feat):
        if not torch.is_grad_enabled():
            return False
        return inp_feat.requires_grad or any(p.requires_grad for p in self.parameters())

    def _trunk(self, x):
        # linear_1..3 with leaky_relu(0.02), then linear_4 (no activation)
        for lin in (self.linear_1, self.linear_2, self.linear_3):
            x = F.leaky_relu(lin(x), negative_slope=0.02)
        return self.linear_4(x)


class IMNet(_DecoderBase):
    """models/implicit_net.py:60-98 — 4-layer MLP inp_dim -> 4gf -> 2gf -> gf -> out_dim."""

    def __init__(self, inp_dim, out_dim, gf_dim=64, use_sigmoid=False):
        super(IMNet, self).__init__()
        self.inp_dim = inp_dim
        self.gf_dim = gf_dim
        self.use_sigmoid = use_sigmoid
        self.linear_1 = nn.Linear(self.inp_dim, self.gf_dim * 4, bias=True)
        self.linear_2 = nn.Linear(self.gf_dim * 4, self.gf_dim * 2, bias=True)
        self.linear_3 = nn.Linear(self.gf_dim * 2, self.gf_dim * 1, bias=True)
        self.linear_4 = nn.Linear(self.gf_dim * 1, out_dim, bias=True)
        if self.use_sigmoid:
            self.sigmoid = nn.Sigmoid()
        # same initialisation as the reference (:72-79)
        for lin, mean in ((self.linear_1, 0.0), (self.linear_2, 0.0), (self.linear_3, 0.0),
                          (self.linear_4, 1e-5)):
            nn.init.normal_(lin.weight, mean=mean, std=0.02)
            nn.init.constant_(lin.bias, 0)

    def forward(self, inp_feat):
        if not inp_feat.is_cuda:
            if _cpu_composite_allowed():
                return self.forward_composite(inp_feat)
            raise RuntimeError("IMNet.forward: CUDA tensor required (no CPU path; " + _CPU_HINT + ")")
        if self._needs_autograd(inp_feat):
            return self._forward_train(inp_feat)
        return decoders_forward(inp_feat, prob_dec=self)[0]

    def forward_composite(self, inp_feat):
        """The same function in differentiable torch ops (the definition the tests compare with)."""
        y = self._trunk(inp_feat)
        return torch.sigmoid(y) if self.use_sigmoid else _leaky_clamp(y)


class IEF(_DecoderBase):
    """models/implicit_net.py:100-152 — iterative error feedback decoder."""

    def __init__(self, device, inp_dim, out_dim, gf_dim=64, n_iter=3, use_sigmoid=False):
        super(IEF, self).__init__()
        self.device = device
        self.init_offset = torch.Tensor([0.001]).float().to(self.device)
        self._init_offset_f = 0.001   # host copy: no device read per call
        self.inp_dim = inp_dim
        self.gf_dim = gf_dim
        self.n_iter = n_iter
        self.use_sigmoid = use_sigmoid
        self.offset_enc = nn.Linear(1, 16, bias=True)
        self.linear_1 = nn.Linear(self.inp_dim + 16, self.gf_dim * 4, bias=True)
        self.linear_2 = nn.Linear(self.gf_dim * 4, self.gf_dim * 2, bias=True)
        self.linear_3 = nn.Linear(self.gf_dim * 2, self.gf_dim * 1, bias=True)
        self.linear_4 = nn.Linear(self.gf_dim * 1, out_dim, bias=True)
        if self.use_sigmoid:
            self.sigmoid = nn.Sigmoid()
        for lin, mean in ((self.offset_enc, 0.0), (self.linear_1, 0.0), (self.linear_2, 0.0),
                          (self.linear_3, 0.0), (self.linear_4, 1e-5)):
            nn.init.normal_(lin.weight, mean=mean, std=0.02)
            nn.init.constant_(lin.bias, 0)

    def forward(self, inp_feat):
        if not inp_feat.is_cuda:
            if _cpu_composite_allowed():
                return self.forward_composite(inp_feat)
            raise RuntimeError("IEF.forward: CUDA tensor required (no CPU path; " + _CPU_HINT + ")")
        if self._needs_autograd(inp_feat):
            return self._forward_train(inp_feat)
        return decoders_forward(inp_feat, offset_dec=self)[1]

    def forward_composite(self, inp_feat):
        """The same function in differentiable torch ops (the definition the tests compare with)."""
        off = self.init_offset.to(inp_feat.device).expand(inp_feat.shape[0], -1)
        for _ in range(self.n_iter):
            off = off + self._trunk(torch.cat([inp_feat, self.offset_enc(off)], 1))
        return torch.sigmoid(off) if self.use_sigmoid else _leaky_clamp(off)
