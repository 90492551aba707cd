"""CLIP ViT-B/32 and ViT-B/16 image encoder on the gfx950 kernels -- drop-in for `perceptor.encode_image`
(AvatarGen/AppearanceGen/main.py:259-260,512,518,524; upstream: OpenAI clip/model.py VisionTransformer, un-vendored).

All GEMMs (patch embedding, in_proj, out_proj, c_fc, c_proj, visual.proj) run in avc_vit_linear / avc_vit_linear_packed (bf16 MFMA,
fp32 accumulate; the reference runs CLIP in fp16 on GPU), attention in avc_vit_attention_*.  Weights are frozen
(`requires_grad_(False)`, main.py:260): the backward only propagates to the pixels, re-using the same GEMM kernel on
the packed transposes.  The twelve residual blocks are one autograd node (BlocksFn) at any batch size; ln_pre / ln_post and the
class-token bookkeeping around them are torch ops under autograd.
Accepts an OpenAI-format state dict (`visual.*` keys, e.g. torch.jit.load('ViT-B-32.pt').state_dict()); the variant -- patch 32 / 50
tokens or patch 16 / 197 tokens, both width 768, 12 layers, 224 x 224 input -- is read from the checkpoint (vision_variant).
"""
import math
import os
from typing import Dict

import torch
import torch.nn.functional as F

from . import lib as L
from . import h2d

WIDTH, LAYERS, HEADS, PATCH, RES, EMBED = 768, 12, 12, 32, 224, 512
TOKENS = (RES // PATCH) ** 2 + 1
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def pack_weight(w: torch.Tensor) -> torch.Tensor:
    """[N,K] -> bf16 [N/32][K/16][64][8] in MFMA B-operand order (lane (n,h) holds W[32t+n][16s+8h+j])."""
    N, K = w.shape
    assert N % 32 == 0 and K % 16 == 0
    p = w.reshape(N // 32, 32, K // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous()
    return p.to(torch.bfloat16).reshape(-1)


VARIANTS = ((32, 50), (16, 197))     # (patch, tokens) of ViT-B/32 and ViT-B/16 at 224 x 224


def vision_variant(state_dict) -> tuple:
    """(patch, tokens) of the image tower in an OpenAI-format CLIP state dict: the patch size from `visual.conv1.weight`, the token
    count from `visual.positional_embedding`.  The kernels are built for width 768, head dim 64 and up to 256 tokens, the host path
    for 12 layers at 224 x 224: ViT-B/32 (32, 50) and ViT-B/16 (16, 197).  Anything else is a ValueError that says what was found."""
    def refuse(found):
        raise ValueError("the CLIP image tower must be ViT-B/32 (patch 32, 50 tokens) or ViT-B/16 (patch 16, 197 tokens) at width %d "
                         "with %d layers; found %s" % (WIDTH, LAYERS, found))
    conv, pos = state_dict.get("visual.conv1.weight"), state_dict.get("visual.positional_embedding")
    if conv is None or pos is None or conv.dim() != 4 or pos.dim() != 2:
        refuse("no ViT image tower (`visual.conv1.weight` [width, 3, patch, patch] and `visual.positional_embedding` [tokens, width]; "
               "a ResNet tower has neither of these shapes)")
    width, patch, tokens = int(conv.shape[0]), int(conv.shape[-1]), int(pos.shape[0])
    layers = len({k.split(".")[3] for k in state_dict if k.startswith("visual.transformer.resblocks.")})
    found = "width %d, patch %d, %d tokens, %d layers" % (width, patch, tokens, layers)
    if width != WIDTH or int(pos.shape[1]) != WIDTH or layers != LAYERS or tuple(conv.shape[1:]) != (3, patch, patch):
        refuse(found)
    if (patch, tokens) not in VARIANTS:
        refuse(found + ("" if patch not in (32, 16) else " (patch %d has (224 / %d)^2 + 1 = %d)" % (patch, patch, (RES // patch) ** 2 + 1)))
    return patch, tokens


TRAIN_GRAPH = os.environ.get("AVC_CLIP_GRAPH", "1") != "0"        # see ClipVisionB32.encode_image


class _Lin:
    def __init__(self, w, b, dev):
        w = w.float().to(dev)
        self.N, self.K = w.shape
        self.wp = pack_weight(w)
        self.wtp = pack_weight(w.t().contiguous())
        self.b = None if b is None else b.float().to(dev).contiguous()


_workspace = {}


def _ws(device, nbytes):
    """bf16 fragment copy of the activations of one avc_vit_linear call (stream-ordered reuse)"""
    key = str(device)
    if key not in _workspace or _workspace[key].numel() < nbytes:
        _workspace[key] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
    return _workspace[key]


BIG_M = 129   # rows from which a call counts as "batched" (3+ images of ViT-B/32, every ViT-B/16 call): the linears then run in the
# LDS-staged GEMM (the C side decides that by itself); up to 128 rows the latency kernel.  BlocksFn runs on either, with and without a
# gradient; which packed operands a call takes: BlocksFn._operands


def _linear_raw(x2d, lin, transposed, bias, residual, act, want_pre, gelu_pre=None):
    """y = x W^T (+ b) (QuickGELU) (+ residual) with bf16 operands and fp32 accumulate / output.  transposed: y = x W (backward);
    gelu_pre (backward only): x is multiplied by QuickGELU'(gelu_pre) first (folded into the packing pass of the kernel)."""
    lib = L.load()
    M = x2d.shape[0]
    N, K = (lin.K, lin.N) if transposed else (lin.N, lin.K)
    wp = lin.wtp if transposed else lin.wp
    y = torch.empty(M, N, device=x2d.device, dtype=torch.float32)
    pre = torch.empty_like(y) if (act and want_pre) else None
    ws = _ws(x2d.device, lib.avc_vit_workspace_bytes(M, K))
    if gelu_pre is not None:
        L.call("avc_vit_linear_bwd_gelu", x2d, gelu_pre, wp, y, M, N, K, ws)
    else:
        L.call("avc_vit_linear", x2d, wp, bias, residual, y, pre, M, N, K, act, ws)
    return y, pre


class LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, lin, act, residual):
        shp = x.shape
        x2 = x.reshape(-1, lin.K).contiguous().float()
        r2 = None if residual is None else residual.reshape(-1, lin.N).contiguous().float()
        # the pre-activation of a QuickGELU layer is only kept for the backward pass (scoring calls run under no_grad: one 4-byte
        # store per output element less)
        y, pre = _linear_raw(x2, lin, False, lin.b, r2, act, bool(act) and ctx.needs_input_grad[0])
        ctx.lin, ctx.act, ctx.has_res = lin, act, residual is not None
        if pre is not None:          # (nothing to save for a linear without activation: a dummy tensor would cost a fill launch per call)
            ctx.save_for_backward(pre)
        return y.reshape(*shp[:-1], lin.N)

    @staticmethod
    def backward(ctx, dy):
        lin = ctx.lin
        shp = dy.shape
        d2 = dy.reshape(-1, lin.N).contiguous().float()
        pre = ctx.saved_tensors[0] if ctx.act else None      # QuickGELU'(pre) is applied inside the GEMM's packing pass
        dx, _ = _linear_raw(d2, lin, True, None, None, 0, False, gelu_pre=pre)
        dres = dy if ctx.has_res else None
        return dx.reshape(*shp[:-1], lin.K), None, None, dres


class AttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv):
        B, T, W3 = qkv.shape          # (the geometry is the tensor's: any T in [1, 256], width = heads * 64)
        qkv = qkv.contiguous().float()
        out = torch.empty(B, T, W3 // 3, device=qkv.device, dtype=torch.float32)
        L.call("avc_vit_attention_fwd", qkv, out, B, T, W3 // 3, W3 // 192)
        ctx.save_for_backward(qkv)
        return out

    @staticmethod
    def backward(ctx, dout):
        (qkv,) = ctx.saved_tensors
        B, T, W3 = qkv.shape
        dout = dout.contiguous().float()
        dqkv = torch.empty_like(qkv)
        L.call("avc_vit_attention_bwd", qkv, dout, dqkv, B, T, W3 // 3, W3 // 192)
        return dqkv


class BlocksFn(torch.autograd.Function):
    """The 12 residual blocks (clip/model.py ResidualAttentionBlock) as ONE autograd node: activations go from kernel to kernel as
    packed bf16 operands -- LayerNorm writes the operand of the linear behind it, attention that of the out-projection, c_fc +
    QuickGELU that of c_proj -- instead of fp32 rows and a packing pass in front of every linear.  The forward serves any number of
    rows, forward and backward: up to 128 (the per-iteration call, 1-2 images of ViT-B/32) on the latency kernel, more (scoring calls:
    ShapeGen/main.py:104-128, pose_generation.py:79-110; every ViT-B/16 call, 197 rows an image; the 5-view batches of AvatarAnimate's
    CLIP-guided optimisers) on the LDS-staged GEMM; avc_vit_linear_packed chooses.  In the backward the proj^T product leaves already
    multiplied by QuickGELU' and packed, and the LayerNorm backward adds the residual branch's gradient and packs its result for the
    transposed linear below.  7 + 8 launches per block instead of 11 + ~14 (a packing launch per linear, torch LayerNorm kernels,
    AccumulateGrad adds).  Arithmetic as in LinearFn / AttentionFn / F.layer_norm: bf16 operands, fp32 accumulation, fp32 residual
    stream and LayerNorm statistics."""

    @staticmethod
    def _operands(model, B, M, keep):
        """(allocator, prefix of the role names) of a call's packed operands.  Up to 128 rows, and every gradient call of 1-2 images
        (what encode_image captures as HIP graphs: 197 / 394 rows of ViT-B/16), the per-shape buffers that are never re-allocated --
        a captured launch must not point at a buffer that a later, larger call replaces.  Everything else one buffer per role grown
        on demand, the gradient calls' under names of their own (a scoring call between a forward and its backward leaves them
        alone).  Rows past M of a grown buffer hold whatever was there: rows are independent in every kernel, no valid row reads them."""
        if M < BIG_M or (keep and B <= 2):
            return model._train_buf, ""
        return model._packed_buf, ("grad_" if keep else "")

    @staticmethod
    def forward(ctx, x, model):
        st = L.stream()
        B, T = x.shape[0], model.tokens
        M, W = B * T, WIDTH
        x0 = x.reshape(M, W).contiguous().float()
        nb = len(model.blocks)
        dev = x0.device
        keep = ctx.needs_input_grad[0]
        # what the backward reads is kept per block; without one a block writes over the one before it and the residual stream is
        # updated in place, in x0 (the caller's ln_pre output: nobody reads it again)
        qkvs = torch.empty(nb if keep else 1, M, 3 * W, device=dev, dtype=torch.float32)
        x2s = torch.empty(nb if keep else 1, M, W, device=dev, dtype=torch.float32)
        xs = torch.empty(nb, M, W, device=dev, dtype=torch.float32) if keep else x0.unsqueeze(0)   # block outputs (= the next block's input)
        pres = torch.empty(nb, M, 4 * W, device=dev, dtype=torch.float32) if keep else None
        buf, pf = BlocksFn._operands(model, B, M, keep)
        a_ln, a_at, a_fc = buf(pf + "ln", M, W), buf(pf + "attn", M, W), buf(pf + "fc", M, 4 * W)

        def linear(xs_, lin, res, y, y_pre, ys, N, K, act):
            L.call("avc_vit_linear_packed", xs_, lin.wp, lin.b, res, None, y, y_pre, ys, M, N, K, act, stream=st)
        cur = x0
        for i, blk in enumerate(model.blocks):
            k = i if keep else 0
            x2, qkv, out = x2s[k], qkvs[k], xs[k]
            L.call("avc_vit_ln_pack", cur, blk["ln1"][0], blk["ln1"][1], 1e-5, M, W, a_ln, stream=st)
            linear(a_ln, blk["qkv"], None, qkv, None, None, 3 * W, W, 0)
            L.call("avc_vit_attention_fwd_packed", qkv, a_at, B, T, W, HEADS, stream=st)
            linear(a_at, blk["out"], cur, x2, None, None, W, W, 0)
            L.call("avc_vit_ln_pack", x2, blk["ln2"][0], blk["ln2"][1], 1e-5, M, W, a_ln, stream=st)
            linear(a_ln, blk["fc"], None, None, pres[i] if keep else None, a_fc, 4 * W, W, 1)
            linear(a_fc, blk["proj"], x2, out, None, None, W, 4 * W, 0)      # (out may be cur: this launch does not read cur)
            cur = out
        if keep:
            ctx.model, ctx.B = model, B
            ctx.save_for_backward(x0, xs, x2s, qkvs, pres)
        return cur.reshape(B, T, W)

    @staticmethod
    def backward(ctx, g):
        st = L.stream()
        model, B = ctx.model, ctx.B
        x0, xs, x2s, qkvs, pres = ctx.saved_tensors
        T = model.tokens
        M, W = B * T, WIDTH
        dev = x0.device
        g = g.reshape(M, W).contiguous().float()
        buf, pf = BlocksFn._operands(model, B, M, True)
        p_g, p_dh = buf(pf + "g", M, W), buf(pf + "dh", M, 4 * W)
        p_g2, p_dqkv = buf(pf + "g2", M, W), buf(pf + "dqkv", M, 3 * W)
        t768 = torch.empty(5, M, W, device=dev, dtype=torch.float32)
        dy2, da, dy1, bufa, bufb = t768[0], t768[1], t768[2], t768[3], t768[4]

        def linear_t(xs_, lin, gelu_pre, y, ys, N, K, act):
            L.call("avc_vit_linear_packed", xs_, lin.wtp, None, None, gelu_pre, y, None, ys, M, N, K, act, stream=st)
        L.call("avc_vit_pack", g, None, p_g, M, W, stream=st)
        for i in range(len(model.blocks) - 1, -1, -1):
            blk = model.blocks[i]
            xin = x0 if i == 0 else xs[i - 1]
            # c_proj^T, times QuickGELU'(pre), packed for c_fc^T
            linear_t(p_g, blk["proj"], pres[i], None, p_dh, 4 * W, W, 2)
            linear_t(p_dh, blk["fc"], None, dy2, None, W, 4 * W, 0)
            # ln_2 backward + the residual branch's gradient: fp32 (the next residual sum) and packed (out_proj^T)
            L.call("avc_vit_ln_bwd", dy2, x2s[i], blk["ln2"][0], 1e-5, g, bufa, p_g2, M, W, stream=st)
            linear_t(p_g2, blk["out"], None, da, None, W, W, 0)
            L.call("avc_vit_attention_bwd_packed", qkvs[i], da, p_dqkv, B, T, W, HEADS, stream=st)
            linear_t(p_dqkv, blk["qkv"], None, dy1, None, W, 3 * W, 0)
            # ln_1 backward + residual: the gradient of the block's input, packed for the block below
            L.call("avc_vit_ln_bwd", dy1, xin, blk["ln1"][0], 1e-5, bufa, bufb, p_g if i else None, M, W, stream=st)
            g = bufb       # (bufa / bufb are re-used by the block below: each is dead by the time it is written again)
        return g.reshape(B, T, W), None


class ClipVision:
    """`perceptor` stand-in: .encode_image(x[B,3,224,224]) -> [B,512] (differentiable wrt x only).  ViT-B/32 or ViT-B/16, whichever
    the state dict holds (vision_variant): `patch` and `tokens` are attributes of the instance.  `ClipVisionB32` is the same class
    under its first name."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], device="cuda"):
        self.patch, self.tokens = vision_variant(state_dict)         # (on the CPU, before any library load)
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("ClipVisionB32 runs on the MI355X kernels only (no CPU fallback)")
        sd = {k: v for k, v in state_dict.items() if k.startswith("visual.")}
        f = lambda k: sd[k].float().to(dev).contiguous()
        self.device = dev
        self.conv = _Lin(sd["visual.conv1.weight"].reshape(WIDTH, -1), None, dev)
        self.cls = f("visual.class_embedding")
        self.pos = f("visual.positional_embedding")
        self.ln_pre = (f("visual.ln_pre.weight"), f("visual.ln_pre.bias"))
        self.ln_post = (f("visual.ln_post.weight"), f("visual.ln_post.bias"))
        self.blocks = []
        for i in range(LAYERS):
            p = "visual.transformer.resblocks.%d." % i
            self.blocks.append(dict(
                ln1=(f(p + "ln_1.weight"), f(p + "ln_1.bias")), ln2=(f(p + "ln_2.weight"), f(p + "ln_2.bias")),
                qkv=_Lin(sd[p + "attn.in_proj_weight"], sd[p + "attn.in_proj_bias"], dev),
                out=_Lin(sd[p + "attn.out_proj.weight"], sd[p + "attn.out_proj.bias"], dev),
                fc=_Lin(sd[p + "mlp.c_fc.weight"], sd[p + "mlp.c_fc.bias"], dev),
                proj=_Lin(sd[p + "mlp.c_proj.weight"], sd[p + "mlp.c_proj.bias"], dev)))
        self.proj = _Lin(sd["visual.proj"].t().contiguous(), None, dev)
        # the text tower is built on demand from the same state dict (clip_text.ClipTextB32) when it carries one
        self._text_sd = state_dict if "token_embedding.weight" in state_dict else None
        self._text = None
        self._packed = {}
        self._graphed = {}
        self._graph_busy = {}         # batch size -> a replayed forward is waiting for its backward
        self._graph_gen = {}          # batch size -> number of replays so far (a backward checks it still owns the static activations)
        self._warned_busy = False
        self._graph_ws = []           # packing workspaces the captured launches point at

    def eval(self):
        return self

    def requires_grad_(self, flag=False):
        return self

    def cuda(self):
        return self

    def _packed_buf(self, tag, M, K):
        """a packed operand of BlocksFn above 128 rows (scoring calls; gradient calls of 3+ images under "grad_" roles): one per
        role, grown on demand, stream-ordered reuse"""
        need = L.load().avc_vit_workspace_bytes(M, K)
        buf = self._packed.get(tag)
        if buf is None or buf.numel() < need:
            buf = self._packed[tag] = torch.empty(need, dtype=torch.uint8, device=self.device)
        return buf

    def _train_buf(self, tag, M, K):
        """a packed operand of BlocksFn up to 128 rows and of every gradient call of 1-2 images (the per-iteration call): one per
        (role, shape), never re-allocated -- captured graphs point at it; zero-filled once (the attention kernel only writes the
        rows below M)"""
        key = ("train", tag, M, K)
        buf = self._packed.get(key)
        if buf is None:
            buf = self._packed[key] = torch.zeros(L.load().avc_vit_workspace_bytes(M, K), dtype=torch.uint8, device=self.device)
        return buf

    def encode_image(self, image: torch.Tensor) -> torch.Tensor:
        """main.py:512,524.  The per-iteration call (1-2 images WITH a gradient to the pixels) -> the encoder's ~250 forward and ~250
        backward launches replayed as two HIP graphs (torch.cuda.make_graphed_callables: captured once per batch size after three
        warm-up passes; bit-identical results, 3.8 -> 0.34 ms of host time per forward + backward) -- what matters when the ray set
        is small and the iteration is bound by the host's launch rate (the reference's default silhouette mode: 7 000 rays);
        everything else eager, on the routes of _encode_image_eager."""
        B = image.shape[0]
        if (TRAIN_GRAPH and B <= 2 and image.is_cuda and torch.is_grad_enabled() and image.requires_grad
                and tuple(image.shape[1:]) == (3, RES, RES) and not torch.cuda.is_current_stream_capturing()):
            g = self._graphed.get(B)
            if g is None:
                sample = torch.zeros(B, 3, RES, RES, device=self.device, dtype=torch.float32, requires_grad=True)
                try:
                    with torch.cuda.device(self.device):     # (capture streams are created on the CURRENT device)
                        # the captured launches bake in the pointer of the linears' packing workspace: size it for the largest linear of
                        # this pass BEFORE the capture (no growth, i.e. no re-allocation, while launches are being recorded) ...
                        _ws(self.device, L.load().avc_vit_workspace_bytes(B * self.tokens, 4 * WIDTH))
                        g = torch.cuda.make_graphed_callables(self._encode_image_eager, (sample,))
                        # ... and keep that buffer alive for as long as the graphs exist: a later, larger eager call (batched scoring,
                        # M > 128) makes _ws() allocate a new one, and dropping the old one would leave the replays writing into freed memory
                        self._graph_ws.append(_workspace[str(self.device)])
                except Exception as e:      # a capture that the runtime refuses must not take the training run down: eager launches
                    import logging
                    logging.warning("CLIP encode_image: HIP graph capture failed (%s: %s); launching eagerly", type(e).__name__, str(e)[:200])
                    g = False
                self._graphed[B] = g
            # One captured instance per batch size = ONE set of static activations: a second call before the first one's backward would
            # overwrite them (and its embedding, which aliases the graph's static output).  The reference does exactly that when
            # add_no_texture is set (main.py:512 then :524, one image each); Runner merges the two into one B = 2 pass, other
            # callers get the eager launches for the overlapping call.  The instance is free again once its backward has run.
            if g is not False and self._graph_busy.get(B, False) and not self._warned_busy:
                self._warned_busy = True
                import warnings
                warnings.warn("ClipVisionB32.encode_image: the captured graphs for batch %d are still waiting for the backward of an "
                              "earlier call; this call runs as ~500 eager launches (Runner releases the graphs at the start of every "
                              "iteration; other callers: release_graphs())" % B, RuntimeWarning, stacklevel=2)
            if g is not False and not self._graph_busy.get(B, False):
                self._graph_busy[B] = True
                gen = self._graph_gen[B] = self._graph_gen.get(B, 0) + 1
                out = g(image.float())

                def _release(grad, B=B, gen=gen):
                    # the instance's static activations belong to its LATEST replay: a backward that arrives for an earlier one (its
                    # forward was declared finished by release_graphs() and the graph replayed since) would differentiate the newer
                    # call's activations -- silently wrong pixel gradients.  Refuse it.
                    if self._graph_gen[B] != gen:
                        raise RuntimeError("ClipVisionB32: backward of a graph-replayed encode_image (batch %d, replay %d) after release_graphs() "
                                           "and a later replay (%d) overwrote its captured activations; run that backward before the next "
                                           "iteration, or take the loss with TRAIN_GRAPH off" % (B, gen, self._graph_gen[B]))
                    self._graph_busy[B] = False
                    return grad
                out.register_hook(_release)
                return out.clone()       # (its own storage: the static output buffer is rewritten by the next replay)
        return self._encode_image_eager(image)

    def release_graphs(self):
        """Declare every graph-replayed forward of earlier calls finished.  The busy flag of a captured instance is cleared by a hook
        in its backward; a grad-enabled call that never reaches backward (an exception between forward and loss.backward(), a skipped
        non-finite loss, a probe call) would otherwise leave it set for good and every later call would silently take the eager path.
        Callers with a step structure call this where no earlier graph can still be wanted -- Runner.train_clip_iteration at its top."""
        for B in self._graph_busy:
            self._graph_busy[B] = False

    def _blocks_packed(self, x):
        """the residual blocks with packed bf16 hand-offs between the kernels (BlocksFn): the route of every call, with or without a
        gradient to the pixels, at any number of rows"""
        return BlocksFn.apply(x, self)

    def _blocks_per_kernel(self, x):
        """the residual blocks as one autograd node per kernel (fp32 rows + a packing pass in front of every linear, torch LayerNorm):
        no call takes it by default; it is what the tests hold BlocksFn against"""
        for blk in self.blocks:
            y = F.layer_norm(x, (WIDTH,), blk["ln1"][0], blk["ln1"][1], 1e-5)
            a = AttentionFn.apply(LinearFn.apply(y, blk["qkv"], 0, None))
            x = LinearFn.apply(a, blk["out"], 0, x)                      # residual fused in the epilogue
            y = F.layer_norm(x, (WIDTH,), blk["ln2"][0], blk["ln2"][1], 1e-5)
            y = LinearFn.apply(y, blk["fc"], 1, None)                    # QuickGELU fused
            x = LinearFn.apply(y, blk["proj"], 0, x)
        return x

    def _encode_image_eager(self, image: torch.Tensor, blocks=None) -> torch.Tensor:
        """blocks: _blocks_packed or _blocks_per_kernel; None = the route every call is meant to take, the packed one"""
        B, P = image.shape[0], self.patch
        # conv1 (P x P, stride P, no bias) == GEMM over flattened patches in (c, ky, kx) order
        x = image.float().reshape(B, 3, RES // P, P, RES // P, P).permute(0, 2, 4, 1, 3, 5)
        x = x.reshape(B, (RES // P) ** 2, 3 * P * P)
        x = LinearFn.apply(x, self.conv, 0, None)
        x = torch.cat([self.cls.expand(B, 1, WIDTH), x], dim=1) + self.pos
        x = F.layer_norm(x, (WIDTH,), self.ln_pre[0], self.ln_pre[1], 1e-5)
        x = (blocks or self._blocks_packed)(x)
        x = F.layer_norm(x[:, 0, :], (WIDTH,), self.ln_post[0], self.ln_post[1], 1e-5)
        return LinearFn.apply(x, self.proj, 0, None)

    def encode_text(self, tokens):
        """main.py:276,282,288 (start-up only): needs a state dict that carries the text tower (a full OpenAI ViT-B/32
        checkpoint does; the seeded vision-only weights of the benchmark do not)"""
        if self._text is None:
            if self._text_sd is None:
                raise RuntimeError("this perceptor was built from vision-only weights: no text tower to encode prompts with "
                                   "(supply a full CLIP state dict, or cached prompt embeddings to Runner.init_clip)")
            from .clip_text import ClipTextB32
            self._text = ClipTextB32(self._text_sd, self.device)
        return self._text.encode_text(tokens)


ClipVisionB32 = ClipVision       # the class's first name, from when ViT-B/32 was the only tower: every existing call site uses it


def load_state_dict(path: str) -> Dict[str, torch.Tensor]:
    """An OpenAI CLIP ViT-B/32 or ViT-B/16 checkpoint: the TorchScript archive `ViT-B-32.pt` / `ViT-B-16.pt` that `clip.load` downloads,
    a plain `torch.save(model.state_dict())` file, or a .safetensors file with the same key names."""
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path)
    try:
        obj = torch.load(path, map_location="cpu", weights_only=True)     # a plain state dict: no code is executed
    except Exception:
        try:
            obj = torch.jit.load(path, map_location="cpu")                # OpenAI's ViT-B-32.pt / ViT-B-16.pt are TorchScript archives
        except RuntimeError:
            # a pickled module or other arbitrary pickle: executes code from the file, as the reference's clip.load does --
            # only with the explicit opt-in
            if os.environ.get("AVC_ALLOW_UNSAFE_PICKLE") != "1":
                raise RuntimeError("%s is neither a tensors-only checkpoint, a .safetensors file nor a TorchScript archive; loading it "
                                   "would execute pickled code (set AVC_ALLOW_UNSAFE_PICKLE=1 to allow that)" % path)
            obj = torch.load(path, map_location="cpu", weights_only=False)
    sd = obj.state_dict() if hasattr(obj, "state_dict") else obj
    return {k: v for k, v in sd.items() if torch.is_tensor(v)}


def clip_preprocess(img_hw3: torch.Tensor) -> torch.Tensor:
    """main.py:261-267,510-511: RandomResizedCrop(224, scale=(1,1)) of a square image == bilinear resize
    (align_corners=False, no antialias); RandomPerspective(p=0) == identity; then Normalize."""
    x = img_hw3.permute(2, 0, 1).unsqueeze(0)
    if x.shape[-1] != RES or x.shape[-2] != RES:
        x = F.interpolate(x, size=(RES, RES), mode="bilinear", align_corners=False)
    mean = h2d.const(CLIP_MEAN, x.device, x.dtype).view(1, 3, 1, 1)
    std = h2d.const(CLIP_STD, x.device, x.dtype).view(1, 3, 1, 1)
    return (x - mean) / std
