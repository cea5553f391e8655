"""RISEv3 policy/value network under PyTorch-ROCm (the evaluator behind the Engine seam).

Architecture follows the reference definition (src/architectures/rise_mobile_v3.py:105-230, 820-849;
builder_util.py:49-80, 154-178, 246-326, 445-483) with the factory arguments of
src/training/train_loop.py:95-116 (shared policy trunk, WDL + plys-to-end heads).  Module and
parameter names match the reference so a reference ``state_dict`` loads unchanged
(``RiseV3.load_state_dict``).  ``InferenceNet`` is the deployed form: BatchNorm folded into the
convolutions, ECA's length-1 Conv1d reduced to its centre tap, channels-last fp16, optional HIP-graph
replay; it returns exactly the tensors the reference's TensorRT engine exposes
(nn/engine.cc:444-461): value, pi_a, pi_b, wdl (loss, draw, win logits), moves_left.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

NB_INPUT_CHANNELS, POLICY_CHANNELS = 74, 73


class _Stem(nn.Module):
    def __init__(self, channels, nb_input_channels):
        super().__init__()
        self.body = nn.Sequential(nn.Conv2d(nb_input_channels, channels, 3, padding=1, bias=False),
                                  nn.BatchNorm2d(channels), nn.ReLU())

    def forward(self, x):
        return self.body(x)


class _ECA(nn.Module):
    """_EfficientChannelAttentionModule with hard-sigmoid (builder_util.py:49-80, :460)."""

    def __init__(self, channels, gamma=2, b=1):
        super().__init__()
        t = int(abs((math.log(channels, 2) + b) / gamma))
        k = t if t % 2 else t + 1
        self.body = nn.Sequential(nn.Conv1d(channels, channels, k, padding=k // 2, bias=True), nn.Hardsigmoid())

    def forward(self, x):
        n, c = x.shape[:2]
        g = self.body(x.mean(dim=(2, 3)).view(n, c, 1)).view(n, c, 1, 1)
        return x * g


class _Bottleneck(nn.Module):
    """_BottlekneckResidualBlock (builder_util.py:445-483): SE gates the block INPUT."""

    def __init__(self, channels, channels_operating, kernel, se):
        super().__init__()
        self.se_type = "eca_se" if se else None
        if se:
            self.se = _ECA(channels)
        self.body = nn.Sequential(
            nn.Conv2d(channels, channels_operating, 1, bias=False), nn.BatchNorm2d(channels_operating), nn.ReLU(),
            nn.Conv2d(channels_operating, channels_operating, kernel, padding=kernel // 2, bias=False, groups=channels_operating),
            nn.BatchNorm2d(channels_operating), nn.ReLU(),
            nn.Conv2d(channels_operating, channels, 1, bias=False), nn.BatchNorm2d(channels))

    def forward(self, x):
        if self.se_type:
            x = self.se(x)
        return x + self.body(x)


class _ValueHead(nn.Module):
    def __init__(self, channels, channels_value_head, fc0):
        super().__init__()
        self.body = nn.Sequential(nn.Conv2d(channels, channels_value_head, 1, bias=False),
                                  nn.BatchNorm2d(channels_value_head), nn.ReLU())
        self.nb_flatten = 64 * channels_value_head
        self.body_wdl = nn.Sequential(nn.Linear(self.nb_flatten, 3))
        self.body_plys = nn.Sequential(nn.Linear(self.nb_flatten, 1), nn.Sigmoid())
        # present in the reference module (unused when use_mlp_wdl_ply is False); kept for state_dict parity
        self.body_final = nn.Sequential(nn.Linear(self.nb_flatten, fc0), nn.ReLU(), nn.Linear(fc0, 1), nn.Tanh())

    def forward(self, x):
        x = self.body(x).reshape(-1, self.nb_flatten)
        wdl = self.body_wdl(x)
        plys = self.body_plys(x)
        sm = torch.softmax(wdl, dim=1)
        return sm[:, 2:3] - sm[:, 0:1], wdl, plys


class _SharedPolicyHeads(nn.Module):
    def __init__(self, channels, policy_channels):
        super().__init__()
        self.shared_body = nn.Sequential(nn.Conv2d(channels, channels, 3, padding=1, bias=False),
                                         nn.BatchNorm2d(channels), nn.ReLU())
        self.board_projections = nn.ModuleList([nn.Conv2d(channels, policy_channels, 3, padding=1, bias=False),
                                                nn.Conv2d(channels, policy_channels, 3, padding=1, bias=False)])

    def forward(self, x):
        s = self.shared_body(x)
        return tuple(p(s).reshape(x.shape[0], -1) for p in self.board_projections)


class RiseV3(nn.Module):
    def __init__(self, channels=384, channels_operating_init=256, channel_expansion=64, kernels=None, se=None,
                 channels_value_head=16, value_fc_size=512):
        super().__init__()
        kernels = kernels or [3] * 15
        se = se or [False] * len(kernels)
        blocks, cop = [], channels_operating_init
        for idx, k in enumerate(kernels):
            active = cop - 32 * (idx // 2) if k == 5 else cop          # rise_mobile_v3.py:68-72
            blocks.append(_Bottleneck(channels, active, k, se[idx]))
            cop += channel_expansion
        self.body_spatial = nn.Sequential(_Stem(channels, NB_INPUT_CHANNELS), *blocks)
        self.value_head = _ValueHead(channels, channels_value_head, value_fc_size)
        self.policy_heads = _SharedPolicyHeads(channels, POLICY_CHANNELS)
        self.config = dict(channels=channels, kernels=list(kernels))

    def forward(self, x):
        out = self.body_spatial(x)
        value, wdl, plys = self.value_head(out)
        pi_a, pi_b = self.policy_heads(out)
        return value, pi_a, pi_b, wdl, plys


def rise_v33() -> RiseV3:
    """get_rise_v33_model (rise_mobile_v3.py:820-849): 15 blocks, 384 ch, 14 122 085 parameters."""
    kernels = [3] * 15
    for i in (7, 11, 12, 13):
        kernels[i] = 5
    se = [False] * 15
    for i in (5, 8, 12, 13, 14):
        se[i] = True
    return RiseV3(384, 256, 64, kernels, se, 16, 512)


def rise_v3_small() -> RiseV3:
    """"RISEv3-small" of BASELINE.json configs[2].  The reference has no model of that name
    (SURVEY.md §8d); defined here as the same RiseV3 class with 128 channels and six 3x3 blocks
    (ECA on the last two)."""
    return RiseV3(128, 128, 32, [3] * 6, [False, False, False, False, True, True], 8, 256)


BOARD_CHANNELS = 37          # input planes per board (NB_INPUT_CHANNELS = 2 x 37)


class _CrossBoardAttentionBlock(nn.Module):
    """rise_mobile_v3.py:242-278: both boards are updated from the PREVIOUS tokens of the other board; the memory of a board is the
    other board's 64 tokens followed by the context tokens; memory_norm serves keys and values alike."""

    def __init__(self, dim, heads, mlp_ratio=2):
        super().__init__()
        self.query_norm = nn.LayerNorm(dim)
        self.memory_norm = nn.LayerNorm(dim)
        self.cross_attention = nn.MultiheadAttention(dim, heads, dropout=0.0, batch_first=True)
        self.mlp_norm = nn.LayerNorm(dim)
        self.mlp = nn.Sequential(nn.Linear(dim, dim * mlp_ratio), nn.GELU(), nn.Linear(dim * mlp_ratio, dim))

    def _update(self, tokens, other, context):
        memory = self.memory_norm(torch.cat((other, context), dim=1))
        tokens = tokens + self.cross_attention(self.query_norm(tokens), memory, memory, need_weights=False)[0]
        return tokens + self.mlp(self.mlp_norm(tokens))

    def forward(self, a, b, context):
        return self._update(a, b, context), self._update(b, a, context)


class _PolicyHead(nn.Module):
    """_PolicyHead with select_policy_from_plane (builder_util.py:206-239): 3x3, BatchNorm, ReLU, 3x3 to the policy planes."""

    def __init__(self, channels, policy_channels):
        super().__init__()
        self.body = nn.Sequential(nn.Conv2d(channels, channels, 3, padding=1, bias=False), nn.BatchNorm2d(channels), nn.ReLU(),
                                  nn.Conv2d(channels, policy_channels, 3, padding=1, bias=False))

    def forward(self, x):
        return self.body(x).reshape(x.shape[0], -1)


class CrossBoardRiseV3(RiseV3):
    """CrossBoardRiseV3 (rise_mobile_v3.py:281-412): the RISEv3 trunk, then one token per square and board (1x1 over the trunk
    features and the board's own 37 planes, + position and board embeddings), seven context tokens (pockets, turns, clock), one or two
    cross-attention blocks between the boards, a value fusion over both board maps into the usual value head, and one policy head per
    board on the post-attention maps.  Parameter names mirror the reference; there is no shared policy trunk."""

    def __init__(self, channels=384, channels_operating_init=256, channel_expansion=64, kernels=None, se=None,
                 channels_value_head=16, value_fc_size=512, attention_dim=192, attention_heads=6, attention_layers=2):
        super().__init__(channels, channels_operating_init, channel_expansion, kernels, se, channels_value_head, value_fc_size)
        if attention_layers not in (1, 2):
            raise ValueError("CrossBoardRiseV3 supports one or two attention layers")
        d = attention_dim
        self.board_token_projections = nn.ModuleList([
            nn.Sequential(nn.Conv2d(channels + BOARD_CHANNELS, d, 1, bias=False), nn.BatchNorm2d(d), nn.ReLU()) for _ in range(2)])
        self.position_embedding = nn.Parameter(torch.zeros(1, 64, d))
        self.board_embedding = nn.Parameter(torch.zeros(2, 1, d))
        self.pocket_projection = nn.Linear(5, d)
        self.scalar_projection = nn.Linear(1, d)
        self.context_role_embedding = nn.Parameter(torch.zeros(1, 7, d))
        self.cross_board_blocks = nn.ModuleList([_CrossBoardAttentionBlock(d, attention_heads) for _ in range(attention_layers)])
        self.value_fusion = nn.Sequential(nn.Conv2d(2 * d, channels, 1, bias=False), nn.BatchNorm2d(channels), nn.ReLU())
        self.policy_heads = nn.ModuleList([_PolicyHead(d, POLICY_CHANNELS) for _ in range(2)])
        for e in (self.position_embedding, self.board_embedding, self.context_role_embedding):
            nn.init.trunc_normal_(e, std=0.02)
        self.config.update(attention_dim=d, attention_heads=attention_heads, attention_layers=attention_layers)

    def context_tokens(self, x):
        o = BOARD_CHANNELS
        mean = lambda a, b: x[:, a:b].mean(dim=(2, 3))
        pockets = [self.pocket_projection(v) for v in (mean(12, 17), mean(17, 22), mean(o + 12, o + 17), mean(o + 17, o + 22))]
        scalars = [self.scalar_projection(v) for v in (mean(25, 26), mean(o + 25, o + 26), mean(31, 32))]
        return torch.stack((*pockets, *scalars), dim=1) + self.context_role_embedding

    def tail(self, features, x):
        """Everything after the trunk: features [n, C, 8, 8], x = the input planes."""
        tokens = [proj(torch.cat((features, planes), dim=1)).flatten(2).transpose(1, 2) + self.position_embedding + self.board_embedding[i]
                  for i, (proj, planes) in enumerate(zip(self.board_token_projections, x.split(BOARD_CHANNELS, dim=1)))]
        context = self.context_tokens(x)
        a, b = tokens
        for block in self.cross_board_blocks:
            a, b = block(a, b, context)
        n = x.shape[0]
        map_a, map_b = a.transpose(1, 2).reshape(n, -1, 8, 8), b.transpose(1, 2).reshape(n, -1, 8, 8)
        value, wdl, plys = self.value_head(self.value_fusion(torch.cat((map_a, map_b), dim=1)))
        return value, self.policy_heads[0](map_a), self.policy_heads[1](map_b), wdl, plys

    def forward(self, x):
        return self.tail(self.body_spatial(x), x)


def cross_board_rise_v33(attention_layers=2) -> CrossBoardRiseV3:
    """get_cross_board_rise_v33_model (rise_mobile_v3.py:852-888): the rise_v33 trunk with the cross-board tail."""
    t = rise_v33()
    blocks = list(t.body_spatial)[1:]
    return CrossBoardRiseV3(384, 256, 64, t.config["kernels"], [b.se_type is not None for b in blocks], 16, 512, attention_layers=attention_layers)


def load_checkpoint(path, model: RiseV3 = None, map_location="cpu") -> RiseV3:
    """Trained-weight ingestion: the reference trainer's checkpoint file, written by save_torch_state
    (src/training/trainer_agent.py:871-890) as torch.save({'model_state_dict', 'optimizer_state_dict',
    ['training_iteration', 'evaluation_step', 'batch_steps']}) and restored by restore_torch_state (:866-868) with a strict
    load_state_dict.  A bare state_dict is accepted too; 'module.' / '_orig_mod.' prefixes (DataParallel, torch.compile) are
    stripped.  Returns the model in eval mode, ready for InferenceNet / FusedNet."""
    ckpt = torch.load(path, map_location=map_location, weights_only=False)
    sd = ckpt["model_state_dict"] if isinstance(ckpt, dict) and "model_state_dict" in ckpt else ckpt
    if not isinstance(sd, dict) or not sd:
        raise ValueError(f"{path}: no model_state_dict")
    clean = {}
    for k, v in sd.items():
        for pre in ("module.", "_orig_mod."):
            while k.startswith(pre):
                k = k[len(pre):]
        clean[k] = v
    if model is None:
        ch = clean["body_spatial.0.body.0.weight"].shape[0]
        layers = len({k.split(".")[1] for k in clean if k.startswith("cross_board_blocks.")})       # the reference's loader: src/main.py:31-33
        if layers:
            if ch != 384:
                raise ValueError(f"{path}: a cross-board checkpoint of {ch} channels needs its model passed in")
            model = cross_board_rise_v33(layers)
        else:
            model = rise_v33() if ch == 384 else rise_v3_small()
    model.load_state_dict(clean, strict=True)
    return model.eval()


def flops_per_position(model: RiseV3) -> float:
    """Multiply-accumulate count x2 of the conv / linear layers at 8x8."""
    total = 0
    for m in model.modules():
        if isinstance(m, nn.Conv2d):
            total += 2 * 64 * m.out_channels * (m.in_channels // m.groups) * m.kernel_size[0] * m.kernel_size[1]
        elif isinstance(m, nn.Conv1d):
            total += 2 * m.out_channels * m.in_channels          # centre tap only on a length-1 sequence
        elif isinstance(m, nn.Linear):
            total += 2 * m.in_features * m.out_features
    fin = model.value_head.body_final
    total -= 2 * (fin[0].in_features * fin[0].out_features + fin[2].in_features * fin[2].out_features)
    return float(total)


def _fold(conv: nn.Conv2d, bn: nn.BatchNorm2d):
    w = conv.weight.detach().float()
    scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
    return w * scale.view(-1, 1, 1, 1), bn.bias.detach().float() - bn.running_mean.detach().float() * scale


class InferenceNet(nn.Module):
    """Deployed form of a RiseV3 (eval mode): folded BN, fp16 channels-last, fixed output contract."""

    def __init__(self, model: RiseV3, dtype=torch.float16, device="cuda"):
        super().__init__()
        if isinstance(model, CrossBoardRiseV3):
            raise NotImplementedError("InferenceNet holds plain RISEv3 networks; a CrossBoardRiseV3 runs through FusedNet")
        model = model.eval()
        self.dtype = dtype
        mk = lambda w, b, **kw: (w.to(device=device, dtype=dtype).contiguous(memory_format=torch.channels_last),
                                 b.to(device=device, dtype=dtype), kw)
        stem = model.body_spatial[0].body
        self.stem = mk(*_fold(stem[0], stem[1]), padding=1)
        self.blocks = []
        for blk in list(model.body_spatial)[1:]:
            b = blk.body
            eca = None
            if blk.se_type:
                c1 = blk.se.body[0]
                k = c1.kernel_size[0]
                eca = (c1.weight.detach()[:, :, k // 2].to(device=device, dtype=dtype).contiguous(),
                       c1.bias.detach().to(device=device, dtype=dtype))
            self.blocks.append(dict(
                eca=eca,
                c1=mk(*_fold(b[0], b[1])),
                dw=mk(*_fold(b[3], b[4]), padding=b[3].padding[0], groups=b[3].groups),
                c2=mk(*_fold(b[6], b[7]))))
        vh = model.value_head
        self.vconv = mk(*_fold(vh.body[0], vh.body[1]))
        # fused value-head linear: rows 0..2 = wdl logits, row 3 = plys logit; NCHW flatten order
        # (reference .view(-1, nb_flatten) on an NCHW tensor) is kept by permuting the weight instead
        # of the activation: channels-last activations flatten as (h, w, c).
        wl = torch.cat([vh.body_wdl[0].weight.detach(), vh.body_plys[0].weight.detach()], 0).float()
        cv = vh.body[0].out_channels
        wl = wl.view(4, cv, 64).permute(0, 2, 1).reshape(4, 64 * cv)
        self.vlin_w = wl.to(device=device, dtype=dtype).contiguous()
        self.vlin_b = torch.cat([vh.body_wdl[0].bias.detach(), vh.body_plys[0].bias.detach()]).to(device=device, dtype=dtype)
        ph = model.policy_heads
        self.pshared = mk(*_fold(ph.shared_body[0], ph.shared_body[1]), padding=1)
        wp = torch.cat([ph.board_projections[0].weight.detach(), ph.board_projections[1].weight.detach()], 0).float()
        self.pproj = mk(wp, torch.zeros(wp.shape[0]), padding=1)
        self._graph = None
        self._static_in = None
        self._static_out = None

    @staticmethod
    def _conv(x, p, relu):
        w, b, kw = p
        y = F.conv2d(x, w, b, **kw)
        return F.relu_(y) if relu else y

    def forward(self, planes: torch.Tensor):
        x = planes.to(self.dtype).contiguous(memory_format=torch.channels_last)
        x = self._conv(x, self.stem, True)
        for blk in self.blocks:
            if blk["eca"] is not None:
                w, b = blk["eca"]
                g = F.hardsigmoid(F.linear(x.mean(dim=(2, 3)), w, b))
                x = x * g[:, :, None, None]
            y = self._conv(x, blk["c1"], True)
            y = self._conv(y, blk["dw"], True)
            y = self._conv(y, blk["c2"], False)
            x = x + y
        n = x.shape[0]
        v = self._conv(x, self.vconv, True)
        v = v.permute(0, 2, 3, 1).reshape(n, -1)                     # (h, w, c) flatten, matches vlin_w
        lin = F.linear(v, self.vlin_w, self.vlin_b).float()
        wdl = lin[:, :3]
        sm = torch.softmax(wdl, dim=1)
        value = (sm[:, 2] - sm[:, 0])
        plys = torch.sigmoid(lin[:, 3])
        s = self._conv(x, self.pshared, True)
        p = self._conv(s, self.pproj, False)                          # [n, 146, 8, 8] channels-last
        p = p.contiguous(memory_format=torch.contiguous_format)      # plane-major [73][64] per head
        pi_a = p[:, :POLICY_CHANNELS].reshape(n, -1)
        pi_b = p[:, POLICY_CHANNELS:].reshape(n, -1)
        h = torch.float16
        return (value.to(h).contiguous(), pi_a.to(h).contiguous(), pi_b.to(h).contiguous(),
                wdl.to(h).contiguous(), plys.to(h).contiguous())

    # ---- HIP-graph replay for a fixed batch (launch-bound at small batch) -----------------
    def capture(self, batch: int):
        self._static_in = torch.zeros((batch, NB_INPUT_CHANNELS, 8, 8), dtype=torch.float16, device=self.vlin_w.device)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.no_grad():
            for _ in range(3):
                self.forward(self._static_in)
        torch.cuda.current_stream().wait_stream(s)
        self._graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._graph), torch.no_grad():
            self._static_out = self.forward(self._static_in)
        return self

    @torch.no_grad()
    def __call__(self, planes: torch.Tensor):
        if self._graph is not None and planes.shape == self._static_in.shape:
            self._static_in.copy_(planes)
            self._graph.replay()
            return self._static_out
        return self.forward(planes)


# ---------------------------------------------------------------------------------------------
# Fused single-launch forward (hivemind_amd/csrc/hm_net.hip)
# ---------------------------------------------------------------------------------------------
def _pack_frag(wt: torch.Tensor) -> torch.Tensor:
    """[K, N] (K % 16 == 0, N % 32 == 0) -> v_mfma_f32_32x32x16_f16 fragment order
    [kstep][tile][lane][8]: lane l holds W[kstep*16 + 8*(l>>5) + j][tile*32 + (l&31)]."""
    k, n = wt.shape
    assert k % 16 == 0 and n % 32 == 0, (k, n)
    x = wt.reshape(k // 16, 2, 8, n // 32, 32)          # ks, h, j, t, c
    return x.permute(0, 3, 1, 4, 2).contiguous().reshape(-1)   # ks, t, h, c, j


def quantize_e4m3(w2d: torch.Tensor):
    """[K, N] fp32 (GEMM orientation) -> (codes uint8 [K, N], scale fp32 [N]): OCP e4m3 with one scale per output channel,
    scale[n] = amax_k |w[k, n]| / 448 (448 = the largest e4m3 value, so no code saturates to the NaN pattern).  An all-zero
    column gets scale 1.0 and zero codes."""
    w2d = w2d.detach().float()
    amax = w2d.abs().amax(dim=0)
    scale = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    q = (w2d / scale).clamp(-448.0, 448.0)                # fp32 division may land a hair over 448
    codes = q.to(torch.float8_e4m3fn).view(torch.uint8)
    assert not bool(((codes & 0x7F) == 0x7F).any()), "e4m3 NaN code"
    return codes.contiguous(), scale.contiguous()


def _pack_frag8(codes: torch.Tensor) -> torch.Tensor:
    """[K, N] bytes (K % 32 == 0, N % 32 == 0) -> the fragment order of _pack_frag with two k-steps per lane,
    [kstep/2][tile][lane][2][8]: lane l holds, for k-steps ks = 2p and 2p + 1, W[ks*16 + 8*(l>>5) + j][tile*32 + (l&31)]
    (16 bytes per lane, one coalesced 1 KiB wave-load per k-step pair)."""
    k, n = codes.shape
    assert k % 32 == 0 and n % 32 == 0, (k, n)
    x = codes.reshape(k // 32, 2, 2, 8, n // 32, 32)     # p, u (k-step of the pair), h, j, t, c
    return x.permute(0, 4, 2, 5, 1, 3).contiguous().reshape(-1)   # p, t, h, c, u, j


def _pack_frag8x64(codes: torch.Tensor) -> torch.Tensor:
    """[K, N] bytes (K % 64 == 0, N % 32 == 0) -> the operand order of v_mfma_scale_f32_32x32x64_f8f6f4 as the kernel reads it,
    [K/64][tile][lane][32]: lane l holds W[kstep*64 + 32*(l>>5) + j][tile*32 + (l&31)], j = 0..31 (32 bytes per lane, two 16-byte
    loads; the activation fragment is the same 32 consecutive k values of its LDS row)."""
    k, n = codes.shape
    assert k % 64 == 0 and n % 32 == 0, (k, n)
    x = codes.reshape(k // 64, 2, 32, n // 32, 32)       # ks, h, j, t, c
    return x.permute(0, 3, 1, 4, 2).contiguous().reshape(-1)      # ks, t, h, c, j


def act_scale(amax: float) -> float:
    """The static scale of one quantised activation tensor: the power of two 2^ceil(log2(2 * amax / 448)) (a factor 2 of headroom
    over the calibration maximum; a power of two, so that x * (1 / sa) is exact in fp32 and torch and the kernel draw the same codes)."""
    return 2.0 ** math.ceil(math.log2(2.0 * amax / 448.0)) if amax > 0 else 1.0


def quantize_act_e4m3(x: torch.Tensor, sa: float) -> torch.Tensor:
    """The activation quantisation step of acts="fp8": clamp(x / sa, -448, 448), round-to-nearest-even to OCP e4m3 (uint8 codes)."""
    return (x.float() / sa).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)


@torch.no_grad()
def calibrate_act_scales(model: "RiseV3", planes: torch.Tensor):
    """The 2 * nblocks + 2 activation scales of FusedNet(acts="fp8"), from the maxima of the (BatchNorm-folded = eval-mode) model in
    fp32 on the calibration planes, on the planes' device: per block its input after the ECA gate and its depthwise output, then the
    trunk output and the policy trunk's output."""
    import copy
    m = copy.deepcopy(model).float().eval().to(planes.device)
    x = m.body_spatial[0](planes.float())
    amax = []
    for blk in list(m.body_spatial)[1:]:
        if blk.se_type:
            x = blk.se(x)
        y = blk.body[:6](x)                                       # expand, depthwise (each + BatchNorm, ReLU)
        amax += [x.abs().max(), y.abs().max()]
        x = x + blk.body[6:](y)
    amax += [x.abs().max(), m.policy_heads.shared_body(x).abs().max()]
    return [act_scale(float(a)) for a in amax]


class FusedNet:
    """RiseV3 (eval) -> one hm_net_forward launch per batch.  Same output contract as InferenceNet.
    weights="fp8": the 1x1 expand / project, policy-trunk, policy-projection and value convolutions are stored and fetched as
    e4m3 codes with one fp32 scale per output channel (quantize_e4m3 after BatchNorm folding; hm_net_create_w8); activations stay
    fp16, accumulation fp32.  Such a network runs through the same calls; it has no plan file (save) yet.
    pair=True: the pair form of the forward (hm_net_set_pair: two positions per workgroup, every weight fragment multiplying
    M = 128 rows; fp16 trunks of 64 / 128 channels).  Same results bit for bit; the plan file does not record the form.
    split=2 or 3: the team form (hm_net_set_split: every position of the fp16 384-channel trunk is carried by that many workgroups
    inside the one launch, each streaming its share of the weights).  Same results bit for bit; launches of team-form networks must
    not overlap each other (one stream); split_error() tells whether a launch gave up.
    acts="fp8" (with weights="fp8"; trunks of 128 / 384 channels): the same five GEMM families on the native FP8 MFMA, their
    activations quantised to e4m3 too with one static power-of-two scale per tensor (hm_net_create_a8) — calibrated on
    calibration=planes by calibrate_act_scales, or given as act_scales=[2 * nblocks + 2 powers of two].  Not the default.
    serve=True (acts="fp8" only): the serve form (hm_net_set_serve) — the network can be the evaluator of the single-launch search
    (SearchEngine.search_persistent, the self-play driver's one launch per ply); without it such a network is refused there."""

    MAXB, CIN_PAD = 16, 80

    def __init__(self, model: RiseV3, device="cuda", weights="fp16", pair=False, split=0, max_rows=1024, acts="fp16", calibration=None, act_scales=None, serve=False):
        import ctypes as C
        import numpy as np
        from ._lib import lib, check
        import copy
        if weights not in ("fp16", "fp8"):
            raise ValueError("weights must be 'fp16' or 'fp8'")
        if pair and weights == "fp8":
            raise ValueError("pair=True needs fp16 weights")
        if split and (pair or weights == "fp8"):
            raise ValueError("split needs fp16 weights and pair=False")
        if acts not in ("fp16", "fp8"):
            raise ValueError("acts must be 'fp16' or 'fp8'")
        a8 = acts == "fp8"
        if serve and not a8:
            raise ValueError("serve=True needs weights='fp8' and acts='fp8' (the fp16 forms that can serve the single-launch search do so as they are)")
        self.serve = bool(serve)
        if a8:
            if weights != "fp8":
                raise ValueError("acts='fp8' needs weights='fp8'")
            if pair or split:
                raise ValueError("acts='fp8' has no pair or team form")
            if isinstance(model, CrossBoardRiseV3):
                raise ValueError("a CrossBoardRiseV3 runs with fp16 weights and activations")
            if model.body_spatial[0].body[0].out_channels not in (128, 384):
                raise ValueError("acts='fp8' serves trunks of 128 or 384 channels")
            if act_scales is None and calibration is None:
                raise ValueError("acts='fp8' needs calibration planes or act_scales")
            sa = [float(v) for v in act_scales] if act_scales is not None else calibrate_act_scales(model, calibration)
            if len(sa) != 2 * (len(model.body_spatial) - 1) + 2 or any(not (v > 0 and math.isfinite(v) and math.frexp(v)[0] == 0.5) for v in sa):
                raise ValueError("act_scales must be 2 * nblocks + 2 positive powers of two")
            self.act_scales = sa
        self.weights, self.pair, self.split, self.acts = weights, bool(pair), int(split), acts
        fp8 = weights == "fp8"
        self._C, self._lib, self._check = C, lib, check
        if isinstance(model, CrossBoardRiseV3):
            if fp8 or pair or split:
                raise ValueError("a CrossBoardRiseV3 runs with fp16 weights, pair=False and split=0")
            self._init_xboard(copy.deepcopy(model).cpu().float().eval(), device, int(max_rows))
            return
        model = copy.deepcopy(model).cpu().float().eval()       # packing happens on the host
        halfs, floats, bytes8 = [], [], []
        hoff, foff, boff = [0], [0], [0]

        def addq(wt, si=0):    # fp8: [K, N] -> (byte offset of the packed codes, float offset of the scales)
            codes, scale = quantize_e4m3(wt)
            if a8:             # K padded to the MFMA's 64 with zero rows; the input tensor's scale sa[si] folded into the weight scales
                codes = torch.cat([codes, torch.zeros((-codes.shape[0]) % 64, codes.shape[1], dtype=torch.uint8)])
                scale = scale * sa[si]
            off = boff[0]
            bytes8.append(_pack_frag8x64(codes) if a8 else _pack_frag8(codes))
            boff[0] += codes.numel()
            return off, addf(scale)

        def addh(t):
            t = t.detach().float().reshape(-1)
            pad = (-t.numel()) % 8
            if pad:
                t = torch.cat([t, torch.zeros(pad)])
            off = hoff[0]
            halfs.append(t)
            hoff[0] += t.numel()
            return off

        def addf(t):
            t = t.detach().float().reshape(-1)
            off = foff[0]
            floats.append(t)
            foff[0] += t.numel()
            return off

        def conv3_wt(w, cin_pad=None):          # [co][ci][3][3] -> Wt[(ky*3+kx)*cin + ci][co]
            co, ci = w.shape[:2]
            if cin_pad and cin_pad != ci:
                w = torch.cat([w, torch.zeros(co, cin_pad - ci, 3, 3)], 1)
                ci = cin_pad
            return w.permute(2, 3, 1, 0).reshape(9 * ci, co)

        def padn(wt, n):
            return wt if wt.shape[1] == n else torch.cat([wt, torch.zeros(wt.shape[0], n - wt.shape[1])], 1)

        stem = model.body_spatial[0].body
        w, b = _fold(stem[0], stem[1])
        ch = w.shape[0]
        assert ch % 64 == 0
        desc = dict(C=ch, cin_pad=self.CIN_PAD)
        desc["stem_w"] = addh(_pack_frag(conv3_wt(w, self.CIN_PAD)))
        desc["stem_b"] = addf(b)
        blocks = []
        nb = len(model.body_spatial) - 1
        for bi, blk in enumerate(list(model.body_spatial)[1:]):
            body = blk.body
            w1, b1 = _fold(body[0], body[1])
            wd, b2 = _fold(body[3], body[4])
            w2, b3 = _fold(body[6], body[7])
            cop, k = w1.shape[0], wd.shape[-1]
            assert cop % 32 == 0 and k in (3, 5)
            d = dict(cop=cop, k=k, eca=0, ecaw=0, ecab=0)
            if fp8:
                d["w1"], d["s1"] = addq(w1.reshape(cop, ch).t().contiguous(), 2 * bi)
            else:
                d["w1"] = addh(_pack_frag(w1.reshape(cop, ch).t().contiguous()))
            d["b1"] = addf(b1)
            d["dw"] = addh(wd.reshape(cop, k * k))
            d["b2"] = addf(b2)
            if fp8:
                d["w2"], d["s3"] = addq(w2.reshape(ch, cop).t().contiguous(), 2 * bi + 1)
            else:
                d["w2"] = addh(_pack_frag(w2.reshape(ch, cop).t().contiguous()))
            d["b3"] = addf(b3)
            if blk.se_type:
                c1 = blk.se.body[0]
                kk = c1.kernel_size[0]
                d["eca"] = 1
                d["ecaw"] = addh(c1.weight.detach()[:, :, kk // 2].t().contiguous())     # [ci][co]
                d["ecab"] = addf(c1.bias)
            blocks.append(d)
        assert len(blocks) <= self.MAXB
        vh = model.value_head
        wv, bv = _fold(vh.body[0], vh.body[1])
        cv = wv.shape[0]
        assert cv <= 32
        desc["cv"] = cv
        if fp8:
            desc["v_w"], desc["v_s"] = addq(padn(wv.reshape(cv, ch).t().contiguous(), 32), 2 * nb)
        else:
            desc["v_w"] = addh(_pack_frag(padn(wv.reshape(cv, ch).t().contiguous(), 32)))
        desc["v_b"] = addf(torch.cat([bv, torch.zeros(32 - cv)]))
        desc["vl_w"] = addh(torch.cat([vh.body_wdl[0].weight, vh.body_plys[0].weight], 0))
        desc["vl_b"] = addf(torch.cat([vh.body_wdl[0].bias, vh.body_plys[0].bias]))
        ph = model.policy_heads
        ws, bs = _fold(ph.shared_body[0], ph.shared_body[1])
        if fp8:
            desc["ps_w"], desc["ps_s"] = addq(conv3_wt(ws), 2 * nb)
        else:
            desc["ps_w"] = addh(_pack_frag(conv3_wt(ws)))
        desc["ps_b"] = addf(bs)
        wp = torch.cat([ph.board_projections[0].weight.detach().float(), ph.board_projections[1].weight.detach().float()], 0)
        if fp8:
            desc["pp_w"], desc["pp_s"] = addq(padn(conv3_wt(wp), 160), 2 * nb + 1)
            if a8:
                desc["qinv"] = addf(1.0 / torch.tensor(sa, dtype=torch.float64))
            self._init_w8(desc, blocks, halfs, floats, bytes8, device)
            return
        desc["pp_w"] = addh(_pack_frag(padn(conv3_wt(wp), 160)))
        ints = [desc["C"], len(blocks), desc["cv"], desc["cin_pad"], desc["stem_w"], desc["ps_w"], desc["pp_w"], desc["v_w"],
                desc["vl_w"], desc["stem_b"], desc["ps_b"], desc["v_b"], desc["vl_b"]]
        for i in range(self.MAXB):
            if i < len(blocks):
                d = blocks[i]
                ints += [d["cop"], d["k"], d["eca"], 0, d["w1"], d["dw"], d["w2"], d["ecaw"], d["b1"], d["b2"], d["b3"], d["ecab"]]
            else:
                ints += [0] * 12
        self.desc = np.asarray(ints, dtype=np.int32)
        self.wh = torch.cat(halfs).to(device=device, dtype=torch.float16).contiguous()
        self.wf = torch.cat(floats).to(device=device, dtype=torch.float32).contiguous()
        self.device = self.wh.device
        self._out = {}
        h = C.c_void_p()
        check(lib.hm_net_create(self.desc.ctypes.data, self.desc.size, self.wh.data_ptr(), self.wf.data_ptr(), C.byref(h)))
        self.handle = h            # hm_net*: descriptor on the device, launch geometry resolved once
        if self.pair:
            check(lib.hm_net_set_pair(h, 1))
        if self.split:
            check(lib.hm_net_set_split(h, self.split))

    def _init_xboard(self, model, device, max_rows):
        """CrossBoardRiseV3 -> hm_net_create_xboard: the trunk descriptor of the plain path (value head included, no shared policy trunk)
        and the tail's (hmn::XbDesc, hm_net_xboard_device.hpp).  LayerNorm weights and biases are folded into the matrices that follow
        them (q / k / v, mlp.0), 1/sqrt(head dimension) into q."""
        import numpy as np
        C = self._C
        cfg = model.config
        if cfg["attention_dim"] != 192 or cfg["attention_heads"] != 6:
            raise ValueError("the cross-board kernel serves attention_dim=192 with 6 heads")
        halfs, floats, hoff, foff = [], [], [0], [0]

        def addh(t):
            t = t.detach().float().reshape(-1)
            t = torch.cat([t, torch.zeros((-t.numel()) % 8)])
            halfs.append(t)
            hoff[0] += t.numel()
            return hoff[0] - t.numel()

        def addf(t):
            t = t.detach().float().reshape(-1)
            floats.append(t)
            foff[0] += t.numel()
            return foff[0] - t.numel()

        def conv3_wt(w):                        # [co][ci][3][3] -> Wt[(ky*3+kx)*ci + ci][co], co padded to a multiple of 32
            co, ci = w.shape[:2]
            wt = w.permute(2, 3, 1, 0).reshape(9 * ci, co)
            return torch.cat([wt, torch.zeros(9 * ci, (-co) % 32)], 1)

        lin = lambda w: addh(_pack_frag(w.t().contiguous()))          # Linear weight [out][in] -> packed [K = in][N = out]
        stem = model.body_spatial[0].body
        w, b = _fold(stem[0], stem[1])
        ch = w.shape[0]
        if ch not in (64, 128, 384):
            raise ValueError("the cross-board kernel serves trunks of 64, 128 or 384 channels")
        w = torch.cat([w, torch.zeros(ch, self.CIN_PAD - w.shape[1], 3, 3)], 1)
        ints = [ch, len(model.body_spatial) - 1, 0, self.CIN_PAD, addh(_pack_frag(w.permute(2, 3, 1, 0).reshape(9 * self.CIN_PAD, ch))), 0, 0]
        sb = addf(b)
        blocks = []
        for blk in list(model.body_spatial)[1:]:
            body = blk.body
            w1, b1 = _fold(body[0], body[1])
            wd, b2 = _fold(body[3], body[4])
            w2, b3 = _fold(body[6], body[7])
            cop, k = w1.shape[0], wd.shape[-1]
            assert cop % 32 == 0 and k in (3, 5)
            d = [cop, k, 0, 0, addh(_pack_frag(w1.reshape(cop, ch).t().contiguous())), addh(wd.reshape(cop, k * k)),
                 addh(_pack_frag(w2.reshape(ch, cop).t().contiguous())), 0, addf(b1), addf(b2), addf(b3), 0]
            if blk.se_type:
                c1 = blk.se.body[0]
                d[2], d[7], d[11] = 1, addh(c1.weight.detach()[:, :, c1.kernel_size[0] // 2].t().contiguous()), addf(c1.bias)
            blocks.append(d)
        assert len(blocks) <= self.MAXB
        vh = model.value_head
        wv, bv = _fold(vh.body[0], vh.body[1])
        cv = wv.shape[0]
        assert cv <= 32
        ints[2] = cv
        ints += [addh(_pack_frag(torch.cat([wv.reshape(cv, ch).t(), torch.zeros(ch, 32 - cv)], 1).contiguous())),
                 addh(torch.cat([vh.body_wdl[0].weight, vh.body_plys[0].weight], 0)),
                 sb, 0, addf(torch.cat([bv, torch.zeros(32 - cv)])), addf(torch.cat([vh.body_wdl[0].bias, vh.body_plys[0].bias]))]
        for i in range(self.MAXB):
            ints += blocks[i] if i < len(blocks) else [0] * 12
        self.desc = np.asarray(ints, dtype=np.int32)
        # ---- the tail
        blks = list(model.cross_board_blocks)
        eps = {float(n.eps) for bl in blks for n in (bl.query_norm, bl.memory_norm, bl.mlp_norm)}
        assert len(eps) == 1
        tp_w, tp_b, p1_w, p1_b, p2_w = [], [], [], [], []
        for i in range(2):
            proj = model.board_token_projections[i]
            w, b = _fold(proj[0], proj[1])                          # [192][C + 37][1][1]
            wt = torch.cat([w.reshape(192, ch + BOARD_CHANNELS).t(), torch.zeros(48 - BOARD_CHANNELS, 192)], 0)      # K = C features + 37 planes, padded to C + 48
            tp_w.append(addh(_pack_frag(wt.contiguous())))
            tp_b.append(addf(b))
            body = model.policy_heads[i].body
            w, b = _fold(body[0], body[1])
            p1_w.append(addh(_pack_frag(conv3_wt(w))))
            p1_b.append(addf(b))
            p2_w.append(addh(_pack_frag(conv3_wt(body[3].weight.detach().float()))))
        w, b = _fold(model.value_fusion[0], model.value_fusion[1])
        tail = [ch, len(blks), int(np.float32(eps.pop()).view(np.int32)), 0, *tp_w, *p1_w, *p2_w, lin(w.reshape(ch, 384)), *tp_b, *p1_b, addf(b),
                addf(model.position_embedding), addf(model.board_embedding), addf(model.pocket_projection.weight), addf(model.pocket_projection.bias),
                addf(model.scalar_projection.weight), addf(model.scalar_projection.bias), addf(model.context_role_embedding)]
        for bl in blks + [None] * (2 - len(blks)):
            if bl is None:
                tail += [0] * 12
                continue
            att = bl.cross_attention
            wq, wk, wv_ = att.in_proj_weight.detach().float().split(192)
            bq, bk, bv_ = att.in_proj_bias.detach().float().split(192)
            fold = lambda w, b, norm: (w * norm.weight.detach().float()[None, :], w @ norm.bias.detach().float() + b)
            sc = 1.0 / math.sqrt(192 // 6)
            wq, bq = fold(wq, bq, bl.query_norm)
            wk, bk = fold(wk, bk, bl.memory_norm)
            wv_, bv_ = fold(wv_, bv_, bl.memory_norm)
            w1, b1 = fold(bl.mlp[0].weight.detach().float(), bl.mlp[0].bias.detach().float(), bl.mlp_norm)
            tail += [lin(wq * sc), lin(wk), lin(wv_), lin(att.out_proj.weight), lin(w1), lin(bl.mlp[2].weight),
                     addf(bq * sc), addf(bk), addf(bv_), addf(att.out_proj.bias), addf(b1), addf(bl.mlp[2].bias)]
        self.tail_desc = np.asarray(tail, dtype=np.int32)
        self.channels = ch
        self.wh = torch.cat(halfs).to(device=device, dtype=torch.float16).contiguous()
        self.wf = torch.cat(floats).to(device=device, dtype=torch.float32).contiguous()
        self.device = self.wh.device
        self._out = {}
        h = C.c_void_p()
        self._check(self._lib.hm_net_create_xboard(self.desc.ctypes.data, self.desc.size, self.tail_desc.ctypes.data, self.tail_desc.size,
                                                   self.wh.data_ptr(), self.wf.data_ptr(), max_rows, C.byref(h)))
        self.handle = h
        self.weights = "xboard"                  # no plan file (save)

    def tail(self, features: torch.Tensor, planes: torch.Tensor, out=None):
        """CrossBoardRiseV3 only: the tail kernel alone on trunk features [n, 64, C] fp16 (square-major) and the input planes."""
        if planes.dtype != torch.float16 or not planes.is_contiguous():
            planes = planes.to(torch.float16).contiguous()
        n = planes.shape[0]
        if features.dtype != torch.float16 or not features.is_contiguous() or tuple(features.shape) != (n, 64, self.channels):
            raise ValueError("features must be a contiguous fp16 tensor [n, 64, C]")
        v, a, b, w, m = out if out is not None else self._buffers(n)
        self._check(self._lib.hm_net_xboard_tail(self.handle, features.data_ptr(), planes.data_ptr(), n, v.data_ptr(), a.data_ptr(), b.data_ptr(),
                                                 w.data_ptr(), m.data_ptr(), self._C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return v, a, b, w, m

    def split_error(self) -> int:
        """Blocking: 0 when no launch of the team form has given up, else the code of the first give-up (cleared by this call)."""
        code = self._C.c_int(0)
        self._check(self._lib.hm_net_split_error(self.handle, self._C.byref(code)))
        return code.value

    def _init_w8(self, desc, blocks, halfs, floats, bytes8, device):
        """The fp8 network's descriptor (hmn::NetDescW8, hm_net_w8_device.hpp; acts="fp8": hmn::NetDescA8, hm_net_a8_device.hpp, the
        same with the offset of the 1 / sa table behind the header) and its three parameter buffers."""
        import numpy as np
        C = self._C
        ints = [desc["C"], len(blocks), desc["cv"], desc["cin_pad"], desc["stem_w"], desc["vl_w"], desc["ps_w"], desc["pp_w"], desc["v_w"],
                desc["stem_b"], desc["ps_b"], desc["v_b"], desc["vl_b"], desc["ps_s"], desc["pp_s"], desc["v_s"]]
        a8 = self.acts == "fp8"
        if a8:
            ints += [desc["qinv"], 0]
        for i in range(self.MAXB):
            if i < len(blocks):
                d = blocks[i]
                ints += [d["cop"], d["k"], d["eca"], 0, d["w1"], d["w2"], d["dw"], d["ecaw"], d["b1"], d["b2"], d["b3"], d["ecab"], d["s1"], d["s3"]]
            else:
                ints += [0] * 14
        self.desc = np.asarray(ints, dtype=np.int32)
        self.w8 = torch.cat(bytes8).to(device=device).contiguous()
        self.wh = torch.cat(halfs).to(device=device, dtype=torch.float16).contiguous()
        self.wf = torch.cat(floats).to(device=device, dtype=torch.float32).contiguous()
        self.device = self.wh.device
        self._out = {}
        h = C.c_void_p()
        create = self._lib.hm_net_create_a8 if a8 else self._lib.hm_net_create_w8
        self._check(create(self.desc.ctypes.data, self.desc.size, self.w8.data_ptr(), self.wh.data_ptr(), self.wf.data_ptr(), C.byref(h)))
        self.handle = h
        if self.serve:
            self._check(self._lib.hm_net_set_serve(h, 1))

    def close(self):
        if getattr(self, "handle", None):
            self._lib.hm_net_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def save(self, path: str):
        """Packed-network file (the plan-file counterpart Engine::loadNetwork reads back, nn/engine.cc:290-401)."""
        if self.weights != "fp16":
            raise NotImplementedError("plan files hold fp16 networks only")
        wh = self.wh.cpu().numpy()
        wf = self.wf.cpu().numpy()
        self._check(self._lib.hm_net_save_file(str(path).encode(), self.desc.ctypes.data, self.desc.size, wh.ctypes.data, wh.nbytes,
                                               wf.ctypes.data, wf.nbytes))

    def _buffers(self, n):
        if n not in self._out:
            f = dict(dtype=torch.float16, device=self.device)
            self._out[n] = (torch.empty(n, **f), torch.empty((n, POLICY_CHANNELS * 64), **f), torch.empty((n, POLICY_CHANNELS * 64), **f),
                            torch.empty((n, 3), **f), torch.empty(n, **f))
        return self._out[n]

    def __call__(self, planes: torch.Tensor, out=None, group_rows=None, group=8):
        """out = (value[n], pi_a[n,4672], pi_b[n,4672], wdl[n,3], moves_left[n]) fp16 tensors to fill in place.
        group_rows (int32 CUDA tensor [n / group], from SearchEngine.collect): only the first group_rows[g] rows of
        each group of `group` rows are evaluated; the other rows' outputs are left as they are."""
        if planes.dtype != torch.float16 or not planes.is_contiguous():
            planes = planes.to(torch.float16).contiguous()
        n = planes.shape[0]
        v, a, b, w, m = out if out is not None else self._buffers(n)
        st = torch.cuda.current_stream().cuda_stream
        if group_rows is None:
            self._check(self._lib.hm_net_forward(self.handle, planes.data_ptr(), n, v.data_ptr(), a.data_ptr(), b.data_ptr(), w.data_ptr(),
                                                 m.data_ptr(), self._C.c_void_p(st)))
        else:
            if group_rows.dtype != torch.int32 or group_rows.numel() * group != n or group_rows.device.type != "cuda":
                raise ValueError("group_rows must be an int32 CUDA tensor with n / group entries")
            self._check(self._lib.hm_net_forward_groups(self.handle, planes.data_ptr(), n, group_rows.data_ptr(), group, v.data_ptr(), a.data_ptr(),
                                                        b.data_ptr(), w.data_ptr(), m.data_ptr(), self._C.c_void_p(st)))
        return v, a, b, w, m
