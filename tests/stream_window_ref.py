"""Plain torch restatement of the two per-row stream kernels (csrc/stream.hip: qt_stream_window, qt_stream_rows) and
a toy decoder stack on which the per-row incremental scheme of codec.RowCodecStream is checked against the one-shot
decode in fp64 (tests/test_stream_window_ref.py).  The GPU units compare the kernels with these bit for bit."""
import torch
import torch.nn.functional as F

F64 = torch.float64


# ------------------------------------------------------------------------------------------ the two kernels
def stream_window(hist, x, nrow, begin, rows_per_frame, head):
    """hist [B][H][C], x [B][n][C] -> (xin [B][H+n][C], new hist [B][H][C]); inputs are left unchanged."""
    B, H, C = hist.shape
    n = x.shape[1]
    xin = torch.empty(B, H + n, C, dtype=x.dtype)
    new = torch.empty_like(hist)
    for b in range(B):
        z = head if begin[b] else 0
        xin[b, :H] = 0 if begin[b] else hist[b]
        xin[b, H:] = x[b]
        xin[b, H:H + min(z, n)] = 0
        m = int(nrow[b]) * rows_per_frame
        assert 0 <= m <= n
        new[b] = xin[b, m:m + H]
    return xin, new


def stream_rows(nf, nrow, begin, n):
    """nf [B] -> (pos [B][n], row_len [B][n], new nf [B]), int32."""
    B = nf.shape[0]
    base = torch.tensor([0 if begin[b] else int(nf[b]) for b in range(B)], dtype=torch.int32)
    pos = base[:, None] + torch.arange(n, dtype=torch.int32)[None]
    return pos, pos + 1, base + torch.tensor([int(v) for v in nrow], dtype=torch.int32)


# ------------------------------------------------------------------------------------------ toy stack
def snake(x, al, ib):
    return x + ib * torch.sin(x * al) ** 2


class ToyStack:
    """Causal conv k=3 on the frames, a stateless 2x upsample (transposed conv k = stride = 2), then per rate r a block
    (SnakeBeta, transposed conv k = 2r stride r trimmed by r on both sides, two residual units: SnakeBeta, causal
    conv k=3 dilation d, SnakeBeta, conv k=1, all with biases), then SnakeBeta and a causal conv k=3 to one channel.
    Channels-last [B][T][C], fp64.  As in the codec, a frame is at least as many rows as a beginning row's spurious
    ones at every stage (heads[i] <= rows per frame), so the feed in which a row begins covers them."""

    def __init__(self, seed, c_in=3, c0=8, rates=(2, 3), dils=(1, 3)):
        g = torch.Generator().manual_seed(seed)
        rnd = lambda *s: torch.randn(*s, generator=g, dtype=F64) * 0.5  # noqa: E731
        sn = lambda c: (rnd(c).exp(), 1.0 / (rnd(c).exp() + 1e-9))  # noqa: E731
        self.rates, self.dils = rates, dils
        self.pre = (rnd(c0, c_in, 3), rnd(c0))
        self.ups = (rnd(c0, c0, 2), rnd(c0))
        self.blocks = []
        c = c0
        for r in rates:
            units = [dict(d=d, s1=sn(c // 2), c1=(rnd(c // 2, c // 2, 3), rnd(c // 2)), s2=sn(c // 2),
                          c2=(rnd(c // 2, c // 2, 1), rnd(c // 2))) for d in dils]
            self.blocks.append(dict(r=r, s=sn(c), w=rnd(c, c // 2, 2 * r), b=rnd(c // 2), units=units))
            c //= 2
        self.s_last = sn(c)
        self.last = (rnd(1, c, 3), rnd(1))
        self.up = 2
        for r in rates:
            self.up *= r
        self.heads = [0]
        for r in rates:
            self.heads.append((self.heads[-1] + 1) * r)
        self.look = self.heads[-1]

    # -- one-shot: torch's own padded / transposed convolutions
    @staticmethod
    def _conv1(x, wb, d=1):
        w, b = wb
        return F.conv1d(F.pad(x.transpose(1, 2), ((w.shape[2] - 1) * d, 0)), w, b, dilation=d).transpose(1, 2)

    def forward(self, x):
        """x [B][T][c_in] -> [B][up * T - look]"""
        x = self._conv1(x, self.pre)
        x = F.conv_transpose1d(x.transpose(1, 2), self.ups[0], self.ups[1], stride=2).transpose(1, 2)
        for blk in self.blocks:
            r = blk["r"]
            y = F.conv_transpose1d(snake(x, *blk["s"]).transpose(1, 2), blk["w"], blk["b"], stride=r)
            x = y[..., r:y.shape[-1] - r].transpose(1, 2)
            for u in blk["units"]:
                x = x + self._conv1(snake(self._conv1(snake(x, *u["s1"]), u["c1"], u["d"]), *u["s2"]), u["c2"])
        return self._conv1(snake(x, *self.s_last), self.last)[..., 0]


class ToyRowStream:
    """The per-row incremental decode of a ToyStack: RowCodecStream's scheme with stream_window() as the only place
    where row state enters.  feed(x [B][n][c_in], nrow, begin) -> [B][up * n]; row b's valid samples are
    [look if begin[b] else 0, up * nrow[b])."""

    def __init__(self, stack: ToyStack, B: int, pollute=None):
        self.st, self.B, self.hist = stack, B, {}
        self.pollute = pollute  # generator: new histories start as noise (a pooled slot's leftovers)

    def _window(self, key, x, H, rpf, head, nrow, begin):
        B, _, C = x.shape
        if key not in self.hist:
            self.hist[key] = torch.zeros(B, H, C, dtype=F64) if self.pollute is None else \
                torch.randn(B, H, C, generator=self.pollute, dtype=F64)
        xin, self.hist[key] = stream_window(self.hist[key], x, nrow, begin, rpf, head)
        return xin

    def _causal(self, key, x, wb, d, act, rpf, head, nrow, begin):
        """window, then SnakeBeta on the window (the kernels apply it to the conv's operand as it is staged, so the
        histories hold pre-activation rows and the window's zeros stay zeros: SnakeBeta(0) = 0), then the conv"""
        w, b = wb
        H = (w.shape[2] - 1) * d
        xin = self._window(key, x, H, rpf, head, nrow, begin) if H else x
        if act is not None:
            xin = snake(xin, *act)
        return F.conv1d(xin.transpose(1, 2), w, b, dilation=d).transpose(1, 2)  # no padding: the window holds it

    def feed(self, x, nrow, begin):
        st, n = self.st, x.shape[1]
        a = (nrow, begin)
        x = self._causal("pre", x, st.pre, 1, None, 1, 0, *a)
        x = (torch.einsum("btc,cok->btko", x, st.ups[0]) + st.ups[1]).reshape(self.B, 2 * n, -1)
        for bi, blk in enumerate(st.blocks):
            r, L = blk["r"], x.shape[1]
            xin = snake(self._window(f"t{bi}", x, 1, L // n, st.heads[bi], *a), *blk["s"])
            w = blk["w"]  # [cin][cout][2r]: output row t = input t on taps r.., input t + 1 on taps ..r
            y = torch.einsum("btc,cok->btko", xin[:, :-1], w[:, :, r:]) + \
                torch.einsum("btc,cok->btko", xin[:, 1:], w[:, :, :r]) + blk["b"]
            x = y.reshape(self.B, L * r, -1)
            hd, L = st.heads[bi + 1], L * r
            for ui, u in enumerate(blk["units"]):
                h = self._causal(f"u{bi}.{ui}", x, u["c1"], u["d"], u["s1"], L // n, hd, *a)
                x = x + self._causal(f"v{bi}.{ui}", h, u["c2"], 1, u["s2"], L // n, hd, *a)
        return self._causal("last", x, st.last, 1, st.s_last, x.shape[1] // n, st.heads[-1], *a)[..., 0]
