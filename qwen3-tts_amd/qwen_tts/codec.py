"""Qwen3-TTS-Tokenizer-12Hz decoder on the MI355X kernels.

Replaces `Qwen3TTSTokenizerV2Decoder.forward / chunked_decode` and `Qwen3TTSTokenizerV2Model.decode`
(K = qwen_tts/core/tokenizer_12hz/modeling_qwen3_tts_tokenizer_v2.py :823-895, 992-1022).
Layout: channels-last [B][T][C] end to end, so every Conv1d / ConvTranspose1d is an implicit GEMM on
the weight-tiled MFMA kernel (transposed convs become 1- or 2-tap convs whose N = stride*Cout output
columns are already the time-interleaved samples: no pixel shuffle pass).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List

import torch

from . import _hip
from . import kernels as K


def _w(W, name, dev):
    t = W[name]
    if not isinstance(t, torch.Tensor):
        t = torch.from_numpy(t)
    return t.to(dev).float()


class CodecDecoder:
    def __init__(self, ccfg: dict, weights: Dict[str, torch.Tensor], dtype="bf16", device="cuda", fuse_units=True):
        _hip.lib()
        self.ccfg = ccfg
        # forward(): a residual unit of the 96 / 192-channel blocks runs as one qt_codec_resunit launch (same bits)
        # instead of two qt_gemm calls; off = the two-call route everywhere (the A/B and its equality test)
        self.fuse_units = fuse_units
        self._unit_fused = {}  # (C, dil, B, L, workspace?) -> does forward() take the one-launch unit
        self.d = d = ccfg["decoder_config"]
        self.dev = dev = torch.device(device)
        self.wdt = wdt = torch.bfloat16 if dtype == "bf16" else torch.float32
        self.adt = wdt
        W = weights
        g = lambda n: _w(W, n, dev)  # noqa: E731
        # C1: RVQ codebooks (embedding_sum / clamp(cluster_usage)) and the two 1x1 output projections
        Q = d["num_quantizers"]
        tabs = []
        for q in range(Q):
            grp, j = ("rvq_first", q) if q == 0 else ("rvq_rest", q - 1)
            p = f"decoder.quantizer.{grp}.vq.layers.{j}._codebook"
            tabs.append(g(f"{p}.embedding_sum") / g(f"{p}.cluster_usage").clamp(min=1e-5)[:, None])
        self.tables = torch.stack(tabs).contiguous()
        self.cb_dim = self.tables.shape[-1]
        self.proj_first = K.tile_linear(g("decoder.quantizer.rvq_first.output_proj.weight")[:, :, 0], wdt)
        self.proj_rest = K.tile_linear(g("decoder.quantizer.rvq_rest.output_proj.weight")[:, :, 0], wdt)
        # C2
        self.pre_conv = K.tile_conv(g("decoder.pre_conv.conv.weight"), g("decoder.pre_conv.conv.bias"), wdt)
        # C3
        pt = "decoder.pre_transformer"
        self.hid = d["hidden_size"]
        self.heads = d["num_attention_heads"]
        self.kvh = d["num_key_value_heads"]
        self.hd = self.hid // self.heads
        self.inp = K.tile_linear(g(f"{pt}.input_proj.weight"), wdt, g(f"{pt}.input_proj.bias"))
        self.outp = K.tile_linear(g(f"{pt}.output_proj.weight"), wdt, g(f"{pt}.output_proj.bias"), gamma=g(f"{pt}.norm.weight"))
        self.tnorm = g(f"{pt}.norm.weight").contiguous()
        self.layers = []
        for i in range(d["num_hidden_layers"]):
            p = f"{pt}.layers.{i}"
            self.layers.append(dict(
                qkv=K.tile_linear(torch.cat([g(f"{p}.self_attn.q_proj.weight"), g(f"{p}.self_attn.k_proj.weight"),
                                             g(f"{p}.self_attn.v_proj.weight")]), wdt, gamma=g(f"{p}.input_layernorm.weight")),
                o=K.tile_linear(g(f"{p}.self_attn.o_proj.weight"), wdt),
                gu=K.tile_swiglu(g(f"{p}.mlp.gate_proj.weight"), g(f"{p}.mlp.up_proj.weight"), wdt,
                                 gamma=g(f"{p}.post_attention_layernorm.weight")),
                down=K.tile_linear(g(f"{p}.mlp.down_proj.weight"), wdt),
                ln1=g(f"{p}.input_layernorm.weight").contiguous(), ln2=g(f"{p}.post_attention_layernorm.weight").contiguous(),
                ls1=g(f"{p}.self_attn_layer_scale.scale").contiguous(), ls2=g(f"{p}.mlp_layer_scale.scale").contiguous()))
        self.cos, self.sin = K.rope_tables(self.hd, d["rope_theta"], 512, dev)
        # C4
        self.lat = d["latent_dim"]
        self.ups = []
        for i, f in enumerate(d["upsampling_ratios"]):
            p = f"decoder.upsample.{i}"
            self.ups.append(dict(
                f=f, tconv=K.tile_transconv(g(f"{p}.0.conv.weight"), g(f"{p}.0.conv.bias"), wdt, f),
                dw_w=g(f"{p}.1.dwconv.conv.weight")[:, 0, :].contiguous(), dw_b=g(f"{p}.1.dwconv.conv.bias"),
                ln_w=g(f"{p}.1.norm.weight"), ln_b=g(f"{p}.1.norm.bias"),
                pw1=K.tile_linear(g(f"{p}.1.pwconv1.weight"), wdt, g(f"{p}.1.pwconv1.bias")),
                pw2=K.tile_linear(g(f"{p}.1.pwconv2.weight"), wdt, g(f"{p}.1.pwconv2.bias")),
                gamma=g(f"{p}.1.gamma").contiguous()))
        # C5-C7
        self.conv0 = K.tile_conv(g("decoder.decoder.0.conv.weight"), g("decoder.decoder.0.conv.bias"), wdt)
        ds = d["decoder_dim"]
        self.blocks = []
        snake = lambda p: (torch.exp(g(f"{p}.alpha")).contiguous(),  # noqa: E731
                           (1.0 / (torch.exp(g(f"{p}.beta")) + 1e-9)).contiguous())
        for i, r in enumerate(d["upsample_rates"]):
            p = f"decoder.decoder.{i + 1}.block"
            units = []
            for j, dil in enumerate((1, 3, 9)):
                q = f"{p}.{j + 2}"
                units.append(dict(dil=dil, s1=snake(f"{q}.act1"), s2=snake(f"{q}.act2"),
                                  c1=K.tile_conv(g(f"{q}.conv1.conv.weight"), g(f"{q}.conv1.conv.bias"), wdt, dil),
                                  c2=K.tile_conv(g(f"{q}.conv2.conv.weight"), g(f"{q}.conv2.conv.bias"), wdt)))
            self.blocks.append(dict(r=r, cin=ds // 2 ** i, cout=ds // 2 ** (i + 1), s=snake(f"{p}.0"),
                                    tconv=K.tile_transconv(g(f"{p}.1.conv.weight"), g(f"{p}.1.conv.bias"), wdt, r),
                                    units=units))
        n = len(d["upsample_rates"])
        self.c_last = ds // 2 ** n
        self.s_last = snake(f"decoder.decoder.{n + 1}")
        self.conv_last = K.tile_conv(g(f"decoder.decoder.{n + 2}.conv.weight"), g(f"decoder.decoder.{n + 2}.conv.bias"),
                                     wdt)
        self.total_upsample = int(math.prod(d["upsample_rates"]) * math.prod(d["upsampling_ratios"]))
        self._slots = {}  # (B, max_frames) -> [_StreamSlot]: incremental-decode state reused across streams
        self._row_slots = {}  # (B, max_frames, n_max) -> [_RowStreamSlot]
        self._old_rope = []  # grown-out (cos, sin): captured feed graphs still read them
        torch.cuda.synchronize()

    # ------------------------------------------------------------------------------------------------
    def _conv(self, x, Wt, B, t_in, t_out, t_off, out, cin, epi=_hip.EPI_STORE, act=_hip.ACT_NONE, snake=None):
        K.gemm(x, Wt, out, B * t_out, cin, Wt.N, conv=(t_in, t_out, t_off, getattr(Wt, "dil", 1)), epi=epi, act=act,
               snake=snake)

    def _ensure_rope(self, npos):
        """RoPE tables of at least npos positions.  The outgoing tables stay alive: captured feed graphs read them."""
        if self.cos.shape[0] < npos:
            self._old_rope.append((self.cos, self.sin))
            self.cos, self.sin = K.rope_tables(self.hd, self.d["rope_theta"], npos + 64, self.dev)

    def _fuses(self, un, x, bb, B, L, C) -> bool:
        """Does forward() run this residual unit as one qt_codec_resunit launch: the kernel has the shape, the decoder
        is bf16, and the unit's k = 7 conv goes the implicit-GEMM route today (a short window that goes through
        im2col keeps that route and its bits)."""
        if not self.fuse_units or self.adt != torch.bfloat16:
            return False
        key = (C, un["dil"], B, L, K.active_workspace(self.dev) is not None)  # (im2col needs the workspace)
        hit = self._unit_fused.get(key)
        if hit is None:
            hit = K.codec_resunit_supported(x, bb, B, L, C, un["c1"], un["s1"], un["c2"], un["s2"])
            if hit:
                c1 = un["c1"]
                info = K.gemm_route(x, c1, bb, B * L, C, c1.N, conv=(L, L, -(c1.taps - 1) * un["dil"], un["dil"]),
                                    snake=un["s1"])
                hit = info.route == _hip.ROUTE_IGEMM
            self._unit_fused[key] = hit
        return hit

    def _transformer(self, st, h, n):
        """C3 (K:500-574).  h: [B*n][lat] (adt) -> [B*n][lat] (adt); positions, key counts and K/V caches are st's."""
        dev, R = self.dev, st.B * n
        hid, nh, nkv, D, inter = self.hid, self.heads, self.kvh, self.hd, self.d["intermediate_size"]
        x = torch.empty(R, self.inp.N, dtype=torch.float32, device=dev)
        K.gemm(h, self.inp, x, R, self.lat, self.inp.N)
        pos, meta_b, row_len, caches, Lmax, max_keys = st.bind(n)
        row_start = torch.zeros_like(pos)
        qkv_w = (nh + 2 * nkv) * D
        qkv = torch.empty(R, qkv_w, dtype=torch.float32, device=dev)
        q = torch.empty(R, nh * D, dtype=torch.float32, device=dev)
        att = torch.empty(R, nh * D, dtype=torch.float32, device=dev)
        hmid = torch.empty(R, inter, dtype=torch.float32, device=dev)
        eps, win = self.d["rms_norm_eps"], self.d["sliding_window"]
        for L, (kc, vc) in zip(self.layers, caches):
            K.gemm(x, L["qkv"], qkv, R, hid, qkv_w, rms=True, eps=eps)
            K.qkv_post(qkv, R, nh, nkv, D, None, None, eps, self.cos, self.sin, pos, meta_b, pos, q, kc, vc, Lmax)
            K.attention(q, R, nh, nkv, D, kc, vc, Lmax, meta_b, row_start, row_len, att, max_keys, window=win)
            K.gemm(att, L["o"], x, R, nh * D, hid, colscale=L["ls1"], epi=_hip.EPI_ADD)
            K.gemm(x, L["gu"], hmid, R, hid, inter, rms=True, eps=eps, epi=_hip.EPI_SWIGLU)
            K.gemm(hmid, L["down"], x, R, inter, hid, colscale=L["ls2"], epi=_hip.EPI_ADD)
        y = torch.empty(R, self.lat, dtype=self.adt, device=dev)
        K.gemm(x, self.outp, y, R, hid, self.lat, rms=True, eps=eps)
        return y

    def _walk(self, st, codes: torch.Tensor, n: int):
        """The decoder network, C1-C7, for st.B rows of n frames: codes int32 [B, n, 16] (device) -> clamped PCM
        [B][rows].  forward(), CodecStream and RowCodecStream all decode through this; st (a _Stage) answers what
        differs between them: how a stage's input window is formed, where the transformer's positions and caches come
        from, the decoder blocks' two-tap transposed conv, and whether a residual unit may be one launch.  Graph-
        capturable when st is: no host-side state, shapes fixed by (B, n) and the stage."""
        B, dev, adt = st.B, self.dev, self.adt
        # C1
        o1 = torch.empty(B * n, self.cb_dim, dtype=torch.float32, device=dev)
        o2 = torch.empty_like(o1)
        K.rvq_gather(self.tables, codes.shape[2], 1, self.tables.shape[1], self.cb_dim, codes, B, n, o1, o2)
        cd = self.proj_first.N
        h = torch.empty(B * n, cd, dtype=adt, device=dev)
        K.gemm(o1, self.proj_first, h, B * n, self.cb_dim, cd)
        K.gemm(o2, self.proj_rest, h, B * n, self.cb_dim, cd, epi=_hip.EPI_ADD)
        # C2, C3
        x = st.causal("pre", h, n, self.pre_conv, cd)
        x = self._transformer(st, x, n)
        st.after_c3(n)
        # C4: upsample (1-tap transposed conv, no state) + ConvNeXt (causal depthwise k=7 + LayerNorm, then per row)
        L, C = n, self.lat
        for i, u in enumerate(self.ups):
            f = u["f"]
            y = torch.empty(B * L * f, C, dtype=adt, device=dev)
            self._conv(x, u["tconv"], B, L, L, 0, y, C)
            L *= f
            yin, Hd = st.dw_window(f"dw{i}", y, L, C, u["dw_w"].shape[1] - 1)
            z = torch.empty_like(yin)
            K.dwconv_ln(yin, B, Hd + L, C, u["dw_w"], u["dw_b"], u["ln_w"], u["ln_b"], 1e-6, z)
            if Hd:
                z = z[:, Hd:].contiguous()
            hmid = torch.empty(B * L, u["pw1"].N, dtype=adt, device=dev)
            K.gemm(z, u["pw1"], hmid, B * L, C, u["pw1"].N, act=_hip.ACT_GELU)
            K.gemm(hmid, u["pw2"], y, B * L, u["pw1"].N, C, colscale=u["gamma"], epi=_hip.EPI_ADD)
            x = y
        # C5
        x = st.causal("conv0", x, L, self.conv0, C)
        C = self.d["decoder_dim"]
        # C6
        # every SnakeBeta feeds a conv: applied to the conv's A operand as it is staged (no separate pass)
        for bi, blk in enumerate(self.blocks):
            rows, x = st.tconv2(bi, x, L, C, blk)
            L, C = rows * blk["r"], blk["cout"]
            if L == 0:  # (a stream's first feed of too few rows)
                return torch.zeros(B, 0, dtype=torch.float32, device=dev)
            for ui, un in enumerate(blk["units"]):
                x = st.unit(bi, ui, un, x, L, C)
        # C7
        out = st.causal("last", x, L, self.conv_last, C, len(self.blocks), snake=self.s_last,
                        out=torch.empty(B * L, self.conv_last.N, dtype=torch.float32, device=dev))
        pcm = out[:, 0].contiguous()
        K.clamp_pcm(pcm, pcm.numel(), pcm)
        return pcm.view(B, L)

    def forward(self, codes: torch.Tensor) -> torch.Tensor:
        """codes int [B, T, 16] (device) -> pcm fp32 [B, 1920T-555] (K:868-883)."""
        B, T, _ = codes.shape
        return self._walk(_OneShot(self, B), codes.to(self.dev, torch.int32).contiguous(), T)

    def stream(self, B: int, max_frames: int) -> "CodecStream":
        """A stateful incremental decode of up to max_frames frames (one reference chunk with its context); close() it
        to return its state slot (and the slot's captured feed graphs) to the pool."""
        return CodecStream(self, B, max_frames)

    def row_stream(self, B: int, max_frames: int, n_max: int = 8) -> "RowCodecStream":
        """stream() with a clock per batch row (rows begin, idle and end independently; feeds of up to n_max frames)."""
        return RowCodecStream(self, B, max_frames, n_max)

    def signature(self):
        """What a row-state snapshot (RowCodecStream.export_row) and a VoiceCache bind to: this decoder's weights
        (the object itself), its activation dtype and the geometry of a row's state."""
        d = self.d
        return (id(self), str(self.adt), len(self.layers), self.kvh, self.hd, int(d["sliding_window"]), self.lat,
                int(d["decoder_dim"]), tuple(int(r) for r in d["upsample_rates"]),
                tuple(int(r) for r in d["upsampling_ratios"]))

    def _acquire_slot(self, pools, key, make):
        """A free state slot of pools[key] (self._slots or self._row_slots), reset, or a new one from make()."""
        pool = pools.setdefault(key, [])
        sl = next((s for s in pool if not s.busy), None)
        if sl is None:
            sl = make()
            pool.append(sl)
        else:
            sl.reset()
        sl.busy = True
        return sl

    def chunked_decode(self, codes: torch.Tensor, chunk_size=300, left_context_size=25) -> torch.Tensor:
        """K:885-895 (codes [B, T, 16]; same chunk / left-context semantics, including the >300 quirks)."""
        wavs, start, T = [], 0, codes.shape[1]
        while start < T:
            end = min(start + chunk_size, T)
            ctx = left_context_size if start - left_context_size > 0 else start
            w = self.forward(codes[:, start - ctx:end])
            wavs.append(w[:, ctx * self.total_upsample:])
            start = end
        return torch.cat(wavs, -1)

    def decode(self, audio_codes: torch.Tensor) -> List[torch.Tensor]:
        """Qwen3TTSTokenizerV2Model.decode (K:992-1022): [B, T, 16] -> list of 1-D fp32 wavs (device)."""
        cb = self.tables.shape[1]
        if audio_codes.numel() and (int(audio_codes.min()) < 0 or int(audio_codes.max()) >= cb):
            # the reference's codebook lookup raises on such ids (nn.Embedding / F.embedding IndexError)
            raise ValueError(f"audio codes must lie in [0, {cb}); got [{int(audio_codes.min())}, "
                             f"{int(audio_codes.max())}]")
        if audio_codes.shape[1] == 0:
            return [torch.zeros(0, device=self.dev) for _ in range(audio_codes.shape[0])]
        wav = self.chunked_decode(audio_codes)
        lengths = (audio_codes[..., 0] > 0).sum(1) * self.ccfg["decode_upsample_rate"]
        return [a[:int(l)] for a, l in zip(wav, lengths)]


class _Stage:
    """What CodecDecoder._walk asks of a decode mode.  causal(key, x, L, Wt, cin, k, out, epi, snake): a causal conv
    of L new rows, its input window formed the mode's way (k = decoder blocks passed so far); dw_window: the input of
    C4's depthwise conv and its leading history rows; tconv2: a decoder block's two-tap transposed conv, returning
    (rows out, output); bind(n): the transformer's positions, row_batch, key counts, per-layer (K, V) caches, cache
    length and max_keys; unit: one residual unit."""

    def __init__(self, dec: "CodecDecoder", B: int, slot=None):
        self.dec, self.B, self.slot = dec, B, slot

    def _out(self, rows, Wt):
        return torch.empty(self.B * rows, Wt.N, dtype=self.dec.adt, device=self.dec.dev)

    def unit(self, bi, ui, un, x, L, C, bb=None):
        bb = self.causal(f"u{bi}.{ui}", x, L, un["c1"], C, bi + 1, out=bb, snake=un["s1"])
        return self.causal(f"v{bi}.{ui}", bb, L, un["c2"], C, bi + 1, out=x, epi=_hip.EPI_ADD, snake=un["s2"])

    def after_c3(self, n):
        pass


class _OneShot(_Stage):
    """forward(): the whole sequence at once, so a window's history is implicit zero padding (t_off < 0)."""

    def causal(self, key, x, L, Wt, cin, k=0, out=None, epi=_hip.EPI_STORE, snake=None):
        out = self._out(L, Wt) if out is None else out
        self.dec._conv(x, Wt, self.B, L, L, -(Wt.taps - 1) * getattr(Wt, "dil", 1), out, cin, epi, snake=snake)
        return out

    def dw_window(self, key, y, L, C, H):
        return y, 0

    def tconv2(self, bi, x, L, C, blk):
        y = torch.empty(self.B * (L - 1) * blk["r"], blk["cout"], dtype=self.dec.adt, device=self.dec.dev)
        self.dec._conv(x, blk["tconv"], self.B, L, L - 1, 0, y, C, snake=blk["s"])
        return L - 1, y

    def bind(self, T):
        dec, B, dev = self.dec, self.B, self.dec.dev
        dec._ensure_rope(T)
        pos = torch.arange(T, device=dev, dtype=torch.int32).repeat(B)
        meta_b = torch.arange(B, device=dev, dtype=torch.int32).repeat_interleave(T)
        kc = torch.empty(B, dec.kvh, T, dec.hd, dtype=torch.float32, device=dev)
        return pos, meta_b, pos + 1, [(kc, torch.empty_like(kc))] * len(dec.layers), T, min(dec.d["sliding_window"], T)

    def unit(self, bi, ui, un, x, L, C):
        # x_out is a second buffer (tiles read their neighbours' x rows): x and bb swap roles per fused unit
        bb = torch.empty_like(x)
        if self.dec._fuses(un, x, bb, self.B, L, C):
            K.codec_resunit(x, bb, self.B, L, C, un["c1"], un["s1"], un["c2"], un["s2"])
            return bb
        return super().unit(bi, ui, un, x, L, C, bb)


class _Streamed(_Stage):
    """A feed of an incremental decode: every stage's window is [history | x], the history kept on the state slot."""

    def _hist(self, key, H, C, dtype):
        h = self.slot.hist.get(key)
        if h is None:  # first use on this slot (eager, never inside a capture): zeros = the one-shot zero padding
            h = self.slot.hist[key] = torch.zeros(self.B, H, C, dtype=dtype, device=self.dec.dev)
        return h

    def causal(self, key, x, L, Wt, cin, k=0, out=None, epi=_hip.EPI_STORE, snake=None):
        """x [B][L][cin] new input rows -> [B][L][Wt.N] outputs of the causal conv (history = previous inputs)."""
        H = (Wt.taps - 1) * getattr(Wt, "dil", 1)
        # (a 1-tap conv keeps no state and maps a spurious row to a spurious row: no window)
        xin = self.window(key, x, L, cin, H, k) if H else x
        out = self._out(L, Wt) if out is None else out
        self.dec._conv(xin, Wt, self.B, H + L, L, 0, out, cin, epi=epi, snake=snake)
        return out

    def dw_window(self, key, y, L, C, H):
        return self.window(key, y, L, C, H, 0), H


class _SlotStage(_Streamed):
    """One feed of a CodecStream: all rows on the slot's one frame counter; `first` = the decode's first feed."""

    def __init__(self, cs: "CodecStream", first: bool):
        super().__init__(cs.dec, cs.B, cs.slot)
        self.first = first

    def window(self, key, x, L, C, H, k):
        h = self._hist(key, H, C, x.dtype)
        xin = torch.cat([h, x.view(self.B, L, C)], 1)
        h.copy_(xin[:, -H:])
        return xin

    def tconv2(self, bi, x, n, C, blk):
        """Row t <- inputs t, t + 1: the first feed's n rows give n - 1, a later feed's [last input row | x] gives n."""
        h = self._hist(f"t{bi}", 1, C, x.dtype)
        xin = x.view(self.B, n, C) if self.first else torch.cat([h, x.view(self.B, n, C)], 1)
        xin = xin.contiguous()
        L = xin.shape[1]
        h.copy_(xin[:, -1:])
        out = self._out(L - 1, blk["tconv"])
        if L > 1:
            self.dec._conv(xin, blk["tconv"], self.B, L, L - 1, 0, out, C, snake=blk["s"])
        return L - 1, out

    def bind(self, n):
        dec, B, sl, dev = self.dec, self.B, self.slot, self.dec.dev
        # positions nf .. nf + n - 1 from the slot's device frame counter (a captured feed replays with later ones)
        pos = (torch.arange(n, device=dev, dtype=torch.int32) + sl.nf_dev).repeat(B)
        meta_b = torch.arange(B, device=dev, dtype=torch.int32).repeat_interleave(n)
        return pos, meta_b, pos + 1, zip(sl.kc, sl.vc), sl.Lm, dec.d["sliding_window"]

    def after_c3(self, n):
        self.slot.nf_dev.add_(n)


class _RowStage(_Streamed):
    """One feed of capacity n of a RowCodecStream: windows, positions and clocks per the slot's row table."""

    def __init__(self, rs: "RowCodecStream", n: int):
        super().__init__(rs.dec, rs.B, rs.slot)
        self.heads, self.n = rs.heads, n

    def window(self, key, x, L, C, H, k):
        """[history | x] of one stage per the row table, the history advanced by each row's own rows; a beginning
        row's heads[k] spurious rows read as zeros."""
        h = self._hist(key, H, C, x.dtype)
        xin = torch.empty(self.B, H + L, C, dtype=x.dtype, device=self.dec.dev)
        K.stream_window(h, x, xin, self.B, H, L, C, L // self.n, self.heads[k], self.slot.rows)
        return xin

    def tconv2(self, bi, x, L, C, blk):
        # always in its continuing form: [last input row | x] -> L rows of r samples
        xin = self.window(f"t{bi}", x, L, C, 1, bi)
        y = self._out(L, blk["tconv"])
        self.dec._conv(xin, blk["tconv"], self.B, L + 1, L, 0, y, C, snake=blk["s"])
        return L, y

    def bind(self, n):
        sl = self.slot
        pos = torch.empty(self.B * n, dtype=torch.int32, device=self.dec.dev)
        row_len = torch.empty_like(pos)
        K.stream_rows(sl.nf_dev, sl.rows, self.B, n, pos, row_len)
        return pos, sl.meta_b[n], row_len, zip(sl.kc, sl.vc), sl.Lm, self.dec.d["sliding_window"]


class _StreamSlot:
    """State of one incremental decode, reused by successive CodecStreams of the same (B, max_frames): the K/V caches,
    every stage's input history (updated in place, so captured graphs keep pointing at it), the frame counter as a
    device word, and the feed graphs captured on this slot keyed by (frames per feed, first feed)."""

    def __init__(self, dec: "CodecDecoder", B: int, Lm: int, clocks: int = 1):
        dev = dec.dev
        self.Lm = Lm
        self.kc = [torch.zeros(B, dec.kvh, Lm, dec.hd, dtype=torch.float32, device=dev) for _ in dec.layers]
        self.vc = [torch.zeros_like(k) for k in self.kc]
        self.nf_dev = torch.zeros(clocks, dtype=torch.int32, device=dev)
        self.hist = {}      # stage key -> [B][rows][C]
        self.graphs = {}    # feed key -> (graph, static codes input, static pcm output)
        self.uses = {}
        self.busy = False
        # split-K scratch of this slot's GEMVs: every feed of the slot (eager or captured) uses it, whatever stream
        # or workspace context the caller is in, so a captured feed graph never points at a caller's temporary
        self.ws = K.new_workspace(dev)

    def reset(self):
        for h in self.hist.values():
            h.zero_()
        self.nf_dev.zero_()


class _RowStreamSlot(_StreamSlot):
    """State of one per-row incremental decode, pooled per (B, max_frames, n_max): K/V caches of max_frames + n_max
    positions (a filler row's K/V lands past its row's clock, never on a valid slot), every stage's input history,
    the per-row frame clocks and the row table (nrow, begin) as static device buffers, the feed graphs keyed by the
    feed capacity n alone."""

    def __init__(self, dec: "CodecDecoder", B: int, max_frames: int, n_max: int):
        super().__init__(dec, B, max_frames + n_max, clocks=B)
        self.rows = torch.zeros(2, B, dtype=torch.int32, device=dec.dev)
        self.meta_b = {}    # n -> row_batch [B*n]
        self.table = None   # kernels.CodecRowTable of this slot (export_row / adopt_rows), built on first use

    def reset(self):
        pass  # (a row restarts from the zero state through its own begin, whatever the slot held)


# captured feed graphs (per slot and feed shape, once a shape repeats); QT_CODEC_GRAPH=0 always feeds eagerly (A/B)
CODEC_GRAPH = _hip.lib_knob("QT_CODEC_GRAPH", 1) != 0


class _PooledStream:
    """What CodecStream and RowCodecStream share: a pooled state slot handed back by close(), and feeds that replay
    the slot's captured graph of their shape or run eagerly, capturing a shape on its second use."""

    def close(self):
        if self.slot is not None:
            self.slot.busy = False
            self.slot = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _feed(self, key, codes, compute):
        """compute(codes) -> pcm, the device work of one feed (graph-capturable: no host-side state, shapes fixed by
        key): replayed if the slot holds a graph for key, else run under the slot's workspace."""
        slot = self.slot
        g = slot.graphs.get(key)
        if g is not None:
            g[1].copy_(codes)
            g[0].replay()
            return g[2]
        with K.use_workspace(slot.ws):
            pcm = compute(codes)
            slot.uses[key] = slot.uses.get(key, 0) + 1
            if CODEC_GRAPH and slot.uses[key] >= 2:
                slot.graphs[key] = self._capture(codes, compute)
        return pcm

    def _capture(self, codes, compute):
        # capturing executes nothing: the slot state (histories, caches, clocks) is left as the eager feed left it
        dev = self.dec.dev
        cin = codes.clone()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side), K.capturing():
            with torch.cuda.graph(g, stream=side):
                out = compute(cin)
        torch.cuda.current_stream(dev).wait_stream(side)
        return g, cin, out


class CodecStream(_PooledStream):
    """Stateful incremental form of CodecDecoder.forward: frames are fed as they are generated and
    every output sample is computed once.  After n frames have been fed, samples [0, 1920 n - 555) of
    forward(all n frames) are available -- the same prefix, since every stage only looks back (causal convs,
    sliding-window attention) except the decoder blocks' transposed convs, whose output row t needs input rows t and
    t + 1 (their one-row lookahead is what the 555-sample tail is).  State per stage: the last (taps - 1) x dil input
    rows of every causal conv (zeros at the start = the one-shot zero padding), the last input row of every 2-tap
    transposed conv, the transformer's K/V caches (positions 0.. of this decode, window 72).  The per-row math is
    the one-shot's; only the GEMM row counts differ (results equal up to fp summation order).
    A feed of ~140 small launches is host-bound, so a feed shape seen twice on a state slot is captured into a HIP
    graph (positions come from the slot's device frame counter, histories are updated in place) and replayed.
    close() hands the slot back to the decoder's pool.
    """

    def __init__(self, dec: "CodecDecoder", B: int, max_frames: int):
        self.dec, self.B, self.max_frames = dec, B, max_frames
        dec._ensure_rope(max_frames)
        self.slot = dec._acquire_slot(dec._slots, (B, max_frames), lambda: _StreamSlot(dec, B, max_frames))
        self.nf = 0  # frames fed
        self.pcm = torch.zeros(B, dec.total_upsample * max_frames, dtype=torch.float32, device=dec.dev)
        self.ns = 0  # valid samples in self.pcm

    def feed(self, codes: torch.Tensor) -> int:
        """codes int [B, n, 16] (the next n frames) -> number of valid samples now in self.pcm."""
        dec = self.dec
        n = codes.shape[1]
        if n == 0:
            return self.ns
        if self.nf + n > self.max_frames:
            raise ValueError(f"CodecStream holds {self.max_frames} frames; {self.nf} fed, {n} more given")
        codes = codes.to(dec.dev, torch.int32).contiguous()
        first = self.nf == 0
        pcm = self._feed((n, first), codes, lambda c: dec._walk(_SlotStage(self, first), c, n))
        self.nf += n
        L = pcm.shape[1]
        self.pcm[:, self.ns:self.ns + L] = pcm
        self.ns += L
        return self.ns


# ---------------------------------------------------------------------------------------------------------------
# per-row incremental decode: every batch row its own request clock (continuous batching, TTSModel.serve_stream)
@dataclass
class CodecRowSnapshot:
    """One row's incremental-decode state (RowCodecStream.export_row): the packed block of qt_codec_row_state, the
    row clock p it was taken at, and the signature of the decoder whose state it is."""
    p: int
    nbytes: int
    sig: tuple
    block: torch.Tensor  # uint8 [nbytes], device


class RowCodecStream(_PooledStream):
    """CodecStream with a clock per batch row: feed(codes [B, n, 16], nrow [B], begin [B]) -> pcm [B, 1920 n].

    Row b consumes its first nrow[b] <= n frames (the rest is filler: computed, never entering any state); with
    begin[b] it first restarts from the zero state, whatever the slot held (a request begins with nrow[b] >= 1:
    begin with nrow 0 only resets the row, which must then begin again).  Shapes never depend on row state: every
    transposed conv runs CodecStream's non-first form ([history | x] in, n rows out), so a beginning row's output of
    decoder block i starts with s_i = (s_{i-1} + 1) r_i spurious rows (s_0 = 0: 8 / 45 / 184 / 555 at rates 8, 5, 4,
    3 -- 555 is the one-shot's lookahead).  Every later stage's input window reads them as zeros (qt_stream_window's
    `head`), which is the one-shot's zero padding because SnakeBeta(0) = 0.  The valid samples of row b in a feed
    are [555 if begin[b] else 0, 1920 nrow[b]); concatenated from a begin on they equal forward(codes_b)[:1920 F -
    555].  The row table is a static device buffer uploaded before the feed, so one graph per capacity n serves every
    mix of beginning, continuing, idle and ragged rows."""

    def __init__(self, dec: "CodecDecoder", B: int, max_frames: int, n_max: int = 8):
        self.dec, self.B, self.max_frames, self.n_max = dec, B, max_frames, n_max
        dec._ensure_rope(max_frames + n_max)
        self.slot = dec._acquire_slot(dec._row_slots, (B, max_frames, n_max),
                                      lambda: _RowStreamSlot(dec, B, max_frames, n_max))
        self.nf = [0] * B  # frames on each row's clock
        self.live = [False] * B  # the row has begun on this stream (until then the slot's state is another stream's)
        # spurious leading rows of a beginning row after each decoder block
        self.heads = [0]
        rpf = math.prod(u["f"] for u in dec.ups)
        for blk in dec.blocks:
            self.heads.append((self.heads[-1] + 1) * blk["r"])
            rpf *= blk["r"]
            # the feed in which a row begins (nrow >= 1) must cover its spurious rows: later feeds do not mask
            assert self.heads[-1] <= rpf, (self.heads, rpf)

    # -- row state in and out (the voice cache) ---------------------------------------------
    def _hist_specs(self):
        """(stage key, history rows, channels) of every history a feed keeps, in the walk's order."""
        dec = self.dec
        taps = lambda Wt: (Wt.taps - 1) * getattr(Wt, "dil", 1)  # noqa: E731
        specs = [("pre", taps(dec.pre_conv), dec.proj_first.N)]
        specs += [(f"dw{i}", u["dw_w"].shape[1] - 1, dec.lat) for i, u in enumerate(dec.ups)]
        specs.append(("conv0", taps(dec.conv0), dec.lat))
        C = dec.d["decoder_dim"]
        for bi, blk in enumerate(dec.blocks):
            specs.append((f"t{bi}", 1, C))
            C = blk["cout"]
            for ui, un in enumerate(blk["units"]):
                specs += [(f"u{bi}.{ui}", taps(un["c1"]), C), (f"v{bi}.{ui}", taps(un["c2"]), C)]
        specs.append(("last", taps(dec.conv_last), C))
        return [sp for sp in specs if sp[1] > 0]  # (a 1-tap conv keeps no history)

    def _state_table(self):
        """The slot's qt_codec_row_state table, built once per slot.  The histories are created lazily by the first
        feed: they are created here first (zeros, as that feed would), so a fresh slot can adopt."""
        sl, dec, B = self.slot, self.dec, self.B
        if sl.table is None:
            specs = self._hist_specs()
            for key, H, C in specs:
                if key not in sl.hist:
                    sl.hist[key] = torch.zeros(B, H, C, dtype=dec.adt, device=dec.dev)
            if sorted(sl.hist) != sorted(k for k, _, _ in specs) or \
                    any(tuple(sl.hist[k].shape) != (B, H, C) or sl.hist[k].dtype != dec.adt for k, H, C in specs):
                raise RuntimeError("RowCodecStream: the slot's histories are not those of _hist_specs()")
            sl.table = K.CodecRowTable([sl.hist[k] for k, _, _ in specs], sl.kc, sl.vc, sl.nf_dev,
                                       dec.d["sliding_window"])
        return sl.table

    def snapshot_bytes(self) -> int:
        return self._state_table().block_bytes

    def export_row(self, b: int) -> CodecRowSnapshot:
        """The complete state of row b (which has begun on this stream) as a snapshot: one launch on the current
        stream.  The row goes on unchanged."""
        if not 0 <= b < self.B or not self.live[b]:
            raise ValueError(f"row {b} has not begun on this stream: nothing to export")
        tab = self._state_table()
        block = torch.zeros(tab.block_bytes, dtype=torch.uint8, device=self.dec.dev)
        K.codec_row_state(tab, [(block, b, self.nf[b], _hip.CODEC_ROW_EXPORT)])
        return CodecRowSnapshot(self.nf[b], tab.block_bytes, self.dec.signature(), block)

    def adopt_row(self, b: int, snapshot: CodecRowSnapshot):
        self.adopt_rows([(b, snapshot)])

    def adopt_rows(self, pairs):
        """Put snapshots into rows -- pairs = [(row, snapshot)], all in one launch on the current stream.  Each row
        becomes a continuing row at the snapshot's clock p, whatever it held: its spurious head rows were masked in
        the feed that began it on the exporting stream, so the next feed's valid samples are [0, 1920 nrow), the
        first 555 of which belong to the frame before p."""
        jobs = []
        for b, sn in pairs:
            if not isinstance(sn, CodecRowSnapshot) or sn.sig != self.dec.signature():
                raise ValueError("the snapshot is another decoder's row state (weights, dtype or geometry differ)")
            if not 0 <= b < self.B:
                raise ValueError(f"row {b} outside [0, {self.B})")
            if not 1 <= sn.p <= self.max_frames:
                raise ValueError(f"a snapshot at clock {sn.p} does not fit a stream of {self.max_frames} frames per "
                                 "row (a row's state begins with its first frame)")
            jobs.append((sn.block, b, sn.p, _hip.CODEC_ROW_ADOPT))
        if len({j[1] for j in jobs}) != len(jobs):
            raise ValueError("two snapshots for one row")
        tab = self._state_table()
        if any(sn.nbytes != tab.block_bytes for _, sn in pairs):
            raise ValueError("the snapshot's size is not this decoder's")
        K.codec_row_state(tab, jobs)
        for b, sn in pairs:
            self.nf[b], self.live[b] = sn.p, True

    # -- feeding ---------------------------------------------------------------------------------------
    def feed(self, codes: torch.Tensor, nrow, begin) -> torch.Tensor:
        """codes int [B, n, 16]; nrow[b] <= n frames of row b are consumed, after a restart when begin[b].  Returns
        pcm fp32 [B, 1920 n] (valid until the next feed of this capacity); row b's valid samples are
        [555 if begin[b] else 0, 1920 nrow[b])."""
        dec, B, dev, slot = self.dec, self.B, self.dec.dev, self.slot
        n = codes.shape[1]
        nrow, begin = [int(v) for v in nrow], [int(bool(v)) for v in begin]
        if codes.shape[0] != B or len(nrow) != B or len(begin) != B or not 0 < n <= self.n_max:
            raise ValueError(f"RowCodecStream({B} rows, capacity {self.n_max}): got codes {tuple(codes.shape)}")
        for b in range(B):
            if not 0 <= nrow[b] <= n:
                raise ValueError(f"row {b}: nrow {nrow[b]} outside [0, {n}]")
            if nrow[b] and not (begin[b] or self.live[b]):
                raise ValueError(f"row {b} has not begun on this stream")
            if (0 if begin[b] else self.nf[b]) + nrow[b] > self.max_frames:
                raise ValueError(f"RowCodecStream holds {self.max_frames} frames per row; row {b} has "
                                 f"{0 if begin[b] else self.nf[b]}, {nrow[b]} more given")
        codes = codes.to(dev, torch.int32).contiguous()
        # a row that never began on this stream sits on another stream's clock and state: it begins with no frames
        # (clock 0, zero state) until its own begin
        tab = torch.tensor([nrow, [int(begin[b] or not self.live[b]) for b in range(B)]], dtype=torch.int32)
        slot.rows.copy_(tab.pin_memory(), non_blocking=True)
        if n not in slot.meta_b:
            slot.meta_b[n] = torch.arange(B, device=dev, dtype=torch.int32).repeat_interleave(n)
        pcm = self._feed(n, codes, lambda c: dec._walk(_RowStage(self, n), c, n))
        for b in range(B):
            if begin[b]:  # (the spurious rows are masked in the beginning feed only: a begin without frames is a reset)
                self.nf[b], self.live[b] = 0, nrow[b] > 0
            self.nf[b] += nrow[b]
        return pcm
