"""Element-wise float64 tests of the fused BatchNorm kernels (csrc/kernels/bn.hip): forward
statistics, finalize (single, from f64 slot sums, batched), apply, backward reduce / finalize / apply and
the stem's BN + ReLU + MaxPool, at every supported channel count and at the shapes where the launchers take
another path (rows < RPI, one row, ragged chunks, the chunk cap, the grid cap).

The reference is always torch in float64 (tests/bn_cases.py), evaluated on the kernel's own upstream f32
outputs, never another path of the kernel.  On integer data the statistics are exact: mean, dbeta and dres
must match bit for bit, invstd to 8 f32 ulp (rsqrtf), dgamma to 1 ulp; every bf16 output must be the
round-to-nearest-even of the f64 value wherever the f32 arithmetic determines it
(kungfu_amd.utils.numerics.assert_rounds_from), so a failure names the element.  tests/test_bn_cases.py runs
the same assertions on a plain-torch emulation and on eight mutants of it, on the CPU.

Kernel defects found by these tests: none."""
import pytest
import torch

import bn_cases as B

pytestmark = pytest.mark.gpu

CL = torch.channels_last
MOM, EPS = B.MOMENTUM, B.EPS


@pytest.fixture(scope="module")
def H():
    from kungfu_amd._lib import hip

    return hip()


def _dev(t):
    """A CPU integer NCHW tensor as the kernels take it: bf16 channels_last on the GPU."""
    return t.cuda().bfloat16().contiguous(memory_format=CL)


class Case:
    """A bn_cases recipe on the GPU: f32 NCHW tensors for the references, bf16 channels_last for the kernels."""

    def __init__(self, shape, rep=0):
        self.c = B.make_case(shape, rep)
        self.shape, self.rep, self.rows, self.C = shape, rep, self.c["rows"], shape[1]
        for k in ("x", "dy", "res", "dsx"):
            setattr(self, k, self.c[k].cuda())
            setattr(self, k + "b", _dev(self.c[k]))
        for k in ("gamma", "beta", "rm", "rv", "mean", "invstd", "fcoef", "rcoef", "mask"):
            setattr(self, k, self.c[k].cuda())

    def stats(self):
        """Fresh running statistics and a num_batches counter for one call."""
        return self.rm.clone(), self.rv.clone(), torch.tensor([5], dtype=torch.int64, device="cuda")

    def check_finalize(self, what, mean, invstd, coef, rm, rv, nbt, stats_of=None):
        s, q = B.fwd_sums(self.x if stats_of is None else stats_of)
        B.check_finalize(what, s, q, self.rows, self.gamma, self.beta, self.rm, self.rv,
                         (mean, invstd, coef, rm, rv, 5, int(nbt)))


def _same_bits(got, exp, what):
    """Two outputs of two launches agree bit for bit (the raw patterns: neither is a rounded reference)."""
    assert got.dtype == exp.dtype and got.shape == exp.shape, what
    v = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
    bad = got.contiguous().view(v) != exp.contiguous().view(v)
    assert not bad.any(), "%s: %d of %d elements differ; first at %s" % (
        what, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist())


# the batched launches: the three BNs of different C, a full batch of kBnFinMax = 8, and a batch of one
ONE_BN = [((3, 48, 5, 7), 0)]
FIN_BATCHES = {"three": [(s, 0) for s in B.MULTI_FWD], "eight": B.MULTI8_FWD, "one": ONE_BN}
BWD_BATCHES = {"three": [(s, 0) for s in B.MULTI_BWD], "eight": B.MULTI8_BWD, "one": ONE_BN}

FWD_VARIANTS = [("plain", False, False, False), ("relu", True, False, False), ("res", False, True, False),
                ("res_relu", True, True, False), ("res_coef", True, False, True)]


def _forward(H, k, name, relu, res, rc):
    rm, rv, nbt = k.stats()
    y, mean, invstd, coef, mask = H.bn_forward(k.xb, k.resb if (res or rc) else None, k.gamma, k.beta, rm, rv, MOM, EPS,
                                               True, relu, nbt, None, k.rcoef if rc else None)
    what = "%s %s" % (k.shape, name)
    k.check_finalize(what, mean, invstd, coef, rm, rv, nbt)
    assert (mask is not None) == (relu and (res or rc)), what
    B.check_fwd_apply(what, k.x, coef, y, relu, k.res if (res or rc) else None, k.rcoef if rc else None, mask)
    assert y.is_contiguous(memory_format=CL)


@pytest.mark.parametrize("shape", B.UNIT_SHAPES, ids=str)
def test_forward_training(H, shape):
    """Statistics, finalize and apply of bn_forward in training mode: plain, ReLU, residual, residual + ReLU
    (with its mask, bit by bit) and the residual folded through res_coef."""
    k = Case(shape)
    n = 0
    for name, relu, res, rc in FWD_VARIANTS:
        _forward(H, k, name, relu, res, rc)
        n += 1
    assert n == 5


@pytest.mark.parametrize("shape", B.LARGE_SHAPES, ids=str)
def test_relu_at_the_chunk_and_grid_caps(H, shape):
    """More natural chunks than kMaxChunks (the first shape) and more vectors than two per lane of kMaxGrid
    blocks: the second trip and the u = 1 lane of the grid-stride loops of bn_apply_kernel and
    bn_bwd_apply_kernel.  Forward ReLU and backward ReLU on one copy of the recipe."""
    N, C, Hh, W = shape
    assert B.rows_of(shape) * (C // 8) > 2 * 2048 * (256 // (C // 8)) * (C // 8)
    k = Case(shape)
    n = 0
    _forward(H, k, "relu", True, False, False)
    n += 1
    _backward(H, k, "relu_coef")
    n += 1
    assert n == 2


SUMS_SHAPES = [(3, 48, 5, 7), (3, 256, 5, 7), (1, 64, 1, 1), (2, 32, 33, 33)]


@pytest.mark.parametrize("shape", SUMS_SHAPES, ids=str)
def test_forward_from_slot_sums(H, shape):
    """bn_forward(sums=...): exact sums spread unevenly over the 16 f64 slots -- those of another tensor than
    the x of the call, so the outputs show that the slots were used, not a statistics pass over x -- give the
    statistics of that tensor, and every slot is zero afterwards."""
    k = Case(shape)
    s, q = B.fwd_sums(k.dsx)
    n = 0
    for relu in (False, True):
        ws = B.split_slots(s, q, (shape, relu))
        rm, rv, nbt = k.stats()
        y, mean, invstd, coef, _ = H.bn_forward(k.xb, None, k.gamma, k.beta, rm, rv, MOM, EPS, True, relu, nbt, ws)
        what = "%s sums relu=%s" % (shape, relu)
        k.check_finalize(what, mean, invstd, coef, rm, rv, nbt, k.dsx)
        B.check_fwd_apply(what, k.x, coef, y, relu)
        assert not ws.any(), what + ": the slots are not re-zeroed"
        n += 1
    assert n == 2


@pytest.mark.parametrize("batch", list(FIN_BATCHES))
def test_finalize_multi(H, batch):
    """bn_finalize_multi: several BNs of different C finalized by one launch (the narrower ones exit early in
    the blocks past their C), then applied through bn_forward(pre=...), which must not finalize again.
    A batch of one must give, bit for bit, what the single launch of bn_forward(sums=...) gives: the two
    entry points run one body."""
    ks = [Case(s, r) for s, r in FIN_BATCHES[batch]]
    nb = len(ks)
    assert nb == {"three": 3, "eight": 8, "one": 1}[batch] and (nb < 8 or ks[-1].C < max(k.C for k in ks))
    st = [k.stats() for k in ks]
    # not the sums of the xs passed
    wss = [B.split_slots(*B.fwd_sums(k.dsx), ("multi", k.shape) + ((k.rep,) if k.rep else ())) for k in ks]
    single = None
    if nb == 1:
        rm1, rv1, nbt1 = ks[0].stats()
        ws1 = wss[0].clone()
        k = ks[0]
        single = H.bn_forward(k.xb, None, k.gamma, k.beta, rm1, rv1, MOM, EPS, True, True, nbt1, ws1)[:4]
        single += [rm1, rv1, nbt1, ws1]
    outs = H.bn_finalize_multi([k.xb for k in ks], wss, [k.gamma for k in ks], [k.beta for k in ks],
                               [s[0] for s in st], [s[1] for s in st], [s[2] for s in st], [MOM] * nb, [EPS] * nb)
    assert len(outs) == nb
    n = 0
    for k, (rm, rv, nbt), ws, (mean, invstd, coef) in zip(ks, st, wss, outs):
        what = "multi %s %s" % (k.shape, k.rep)
        k.check_finalize(what, mean, invstd, coef, rm, rv, nbt, k.dsx)
        assert not ws.any(), what + ": the slots are not re-zeroed"
        rm1, rv1, coef1 = rm.clone(), rv.clone(), coef.clone()
        y = H.bn_forward(k.xb, None, k.gamma, k.beta, rm, rv, MOM, EPS, True, True, nbt, ws, None, True, None,
                         [mean, invstd, coef])[0]
        assert torch.equal(rm, rm1) and torch.equal(rv, rv1) and torch.equal(coef, coef1) and int(nbt) == 6, what
        B.check_fwd_apply(what, k.x, coef, y, True)
        if single is not None:
            names = ("y", "mean", "invstd", "coef", "running_mean", "running_var", "num_batches", "sums")
            for name, got, exp in zip(names, (y, mean, invstd, coef, rm, rv, nbt, ws), single):
                _same_bits(got, exp, "batch of one against the single launch: " + name)
        n += 1
    assert n == nb


@pytest.mark.parametrize("shape", [(3, 48, 5, 7), (3, 128, 5, 7), (1, 64, 1, 1)], ids=str)
def test_forward_eval(H, shape):
    """Eval mode: coefficients from the running statistics only; running statistics and num_batches untouched."""
    k = Case(shape)
    n = 0
    for relu in (False, True):
        rm, rv, nbt = k.stats()
        y, mean, invstd, coef, _ = H.bn_forward(k.xb, None, k.gamma, k.beta, rm, rv, MOM, EPS, False, relu, nbt)
        what = "%s eval relu=%s" % (shape, relu)
        assert torch.equal(rm, k.rm) and torch.equal(rv, k.rv) and int(nbt) == 5, what
        B.check_eval_coef(what, k.gamma, k.beta, k.rm, k.rv, mean, invstd, coef)
        B.check_fwd_apply(what, k.x, coef, y, relu)
        n += 1
    assert n == 2


@pytest.mark.parametrize("shape,off,tot", [((3, 48, 5, 7), 64, 288), ((3, 96, 5, 7), 0, 160), ((2, 32, 33, 33), 8, 48)],
                         ids=str)
def test_forward_into_a_channel_slice(H, shape, off, tot):
    """out= a channel slice of a wider tensor: the slice holds y, every other channel keeps its sentinel.
    A single variant per case (the launcher takes out= for BN + ReLU without residual only)."""
    k = Case(shape)
    N, C, Hh, W = shape
    big = torch.full((N, tot, Hh, W), 77.0, device="cuda", dtype=torch.bfloat16).contiguous(memory_format=CL)
    rm, rv, nbt = k.stats()
    out = big[:, off:off + C]
    y, mean, invstd, coef, _ = H.bn_forward(k.xb, None, k.gamma, k.beta, rm, rv, MOM, EPS, True, True, nbt, None, None,
                                            True, out)
    what = "%s slice %d of %d" % (shape, off, tot)
    k.check_finalize(what, mean, invstd, coef, rm, rv, nbt)
    B.check_fwd_apply(what, k.x, coef, big[:, off:off + C], True)
    rest = torch.cat([big[:, :off], big[:, off + C:]], 1)
    assert rest.numel() == N * (tot - C) * Hh * W and (rest == 77.0).all(), what + ": a channel outside the slice changed"


# ---- backward --------------------------------------------------------------------------------------

def _backward(H, k, name):
    """One bn_backward variant with the recipe's own mean / invstd / fcoef against the f64 reference."""
    what = "%s %s" % (k.shape, name)
    C = k.C
    on = B.gate(k.x, k.fcoef)[1]
    relu, training, mask, dy, kw = name != "plain", name != "eval", None, k.dyb, {}
    ws = dws = sums = None
    if name == "relu_bits":
        mask = k.mask  # bits unrelated to the gate of fcoef, which is passed all the same
    if name == "strided":
        N, _, Hh, W = k.shape
        big = torch.full((N, C + 40, Hh, W), 3.0, device="cuda", dtype=torch.bfloat16).contiguous(memory_format=CL)
        big[:, 16:16 + C] = k.dyb
        dy = big[:, 16:16 + C]
        assert dy.is_contiguous(memory_format=CL) == (k.rows == 1)  # a single row has no stride to speak of
    if name == "sums":
        # the sums of another gradient than the dy of the call: dgamma / dbeta show whether they were used
        sums = B.bwd_sums(k.res.double() * on, k.x)
        ws = B.split_slots(*sums, ("bwd", k.shape))
        kw["sums"] = ws
    if name == "dres_sums":
        dws = torch.zeros(B.SLOTS * 2 * C, dtype=torch.float64, device="cuda")
        kw["dres_x"], kw["dres_sums"] = k.dsxb, dws
    outs = H.bn_backward(dy, k.xb, k.mean, k.invstd, k.gamma, k.fcoef, mask, relu, training, True, **kw)
    dz = B.check_bwd(what, k.c, "cuda", outs, relu, training, mask, True, sums=sums)
    if ws is not None:
        assert not ws.any(), what + ": the slots are not re-zeroed"
    if dws is not None:
        got = dws.view(B.SLOTS, 2, C).sum(0)
        assert torch.equal(got[0], dz.sum((0, 2, 3))), what + ": sum dres"
        assert torch.equal(got[1], (dz * k.dsx.double()).sum((0, 2, 3))), what + ": sum dres * dres_x"


BWD_VARIANTS = ("plain", "relu_coef", "relu_bits", "eval", "strided", "sums", "dres_sums")


@pytest.mark.parametrize("shape", B.UNIT_SHAPES, ids=str)
def test_backward(H, shape):
    """bn_backward: no ReLU, ReLU from the coefficients, ReLU from mask bits (other bits than the coefficients
    would give), eval mode, a strided dy slice, known sums (of another gradient; consumed and re-zeroed) and the
    second BN's sums of dres (dres_x / dres_sums)."""
    k = Case(shape)
    n = 0
    for name in BWD_VARIANTS:
        _backward(H, k, name)
        n += 1
    assert n == 7


@pytest.mark.parametrize("batch", list(BWD_BATCHES))
def test_backward_multi(H, batch):
    """bn_backward_multi with mixed widths (BNs narrower than the widest: their finalize blocks past C exit
    early), one of the gradients a channel slice of a wider tensor.  A batch of one must give, bit for bit,
    what bn_backward gives: the batched and the single finalize run one body."""
    ks = [Case(s, r) for s, r in BWD_BATCHES[batch]]
    nb = len(ks)
    assert nb == {"three": 3, "eight": 8, "one": 1}[batch] and (nb < 8 or ks[-1].C < max(k.C for k in ks))
    i48 = [k.C for k in ks].index(48)
    N, _, Hh, W = ks[i48].shape
    big = torch.full((N, 48 + 24, Hh, W), 3.0, device="cuda", dtype=torch.bfloat16).contiguous(memory_format=CL)
    big[:, 8:56] = ks[i48].dyb
    dys = [k.dyb for k in ks]
    dys[i48] = big[:, 8:56]
    outs = H.bn_backward_multi(dys, [k.xb for k in ks], [k.mean for k in ks], [k.invstd for k in ks],
                               [k.gamma for k in ks], [k.fcoef for k in ks])
    assert len(outs) == nb
    n = 0
    for k, (dx, dg, db) in zip(ks, outs):
        B.check_bwd("multi %s %s" % (k.shape, k.rep), k.c, "cuda", (dx, None, dg, db), True)
        n += 1
    assert n == nb
    if nb == 1:
        k = ks[0]
        dx1, _, dg1, db1 = H.bn_backward(dys[0], k.xb, k.mean, k.invstd, k.gamma, k.fcoef, None, True, True, False)
        for name, got, exp in zip(("dx", "dgamma", "dbeta"), outs[0], (dx1, dg1, db1)):
            _same_bits(got, exp, "batch of one against bn_backward: " + name)


# ---- stem: BN + ReLU + MaxPool(3, 2, 1) ------------------------------------------------------------

@pytest.mark.parametrize("shape", B.POOL_SHAPES, ids=str)
def test_pool_forward(H, shape):
    """bn_pool_forward: y, the reported window position (inside the image, the maximum, the first of exact
    ties) and xarg = x at that position."""
    k = Case(shape)
    n = 0
    for training in (True, False):
        rm, rv, nbt = k.stats()
        yp, mean, invstd, coef, arg, xarg = H.bn_pool_forward(k.xb, k.gamma, k.beta, rm, rv, MOM, EPS, training, nbt)
        what = "%s pool training=%s" % (shape, training)
        if training:
            k.check_finalize(what, mean, invstd, coef, rm, rv, nbt)
            assert xarg is not None
        else:
            assert torch.equal(rm, k.rm) and torch.equal(rv, k.rv) and int(nbt) == 5, what
            B.check_eval_coef(what, k.gamma, k.beta, k.rm, k.rv, mean, invstd, coef)
        assert tuple(yp.shape) == (shape[0], shape[1], B.pool_out(shape[2]), B.pool_out(shape[3]))
        B.check_pool_fwd(what, k.x, coef, yp, arg, xarg if training else None)
        n += 1
    assert n == 2


@pytest.mark.parametrize("shape", B.POOL_SHAPES, ids=str)
def test_pool_backward(H, shape):
    """bn_pool_backward against an f64 gather reference, with the argmax taken from the f64 reference of the
    recipe's own fcoef: through the full-resolution gather, through the pooled sums (xarg), and apply=False."""
    k = Case(shape)
    N, C, Hh, W = shape
    a = B.first_argmax(k.x, k.fcoef)
    OH, OW = a.shape[2], a.shape[3]
    arg = a.permute(0, 2, 3, 1).contiguous().to(torch.uint8).reshape(-1)
    xarg = B.windows(k.x, 0.0).gather(0, a.unsqueeze(0))[0]
    dyp = B._ints((N, C, OH, OW), False, "dyp", 8, 3).cuda()
    dyfull = B.pool_gather(dyp, a, shape)
    n = 0
    coefs = []
    for name, xa, apply in (("gather", None, True), ("pooled", _dev(xarg), True), ("no apply", _dev(xarg), False)):
        dx, dg, db, coef = H.bn_pool_backward(_dev(dyp), arg, k.xb, k.mean, k.invstd, k.gamma, k.fcoef, True, xa, apply)
        what = "%s pool backward %s" % (shape, name)
        coefs.append((dg, db, coef))
        if apply:
            B.check_bwd(what, k.c, "cuda", (dx, None, dg, db), True, dy=dyfull)
        else:
            assert dx.numel() == 0, what
            assert all(torch.equal(u, v) for u, v in zip(coefs[1], coefs[2])), what + ": other coefficients"
        n += 1
    # the coefficients the apply=False caller consumes: k1 bit for bit, k2 / k3 within the path's roundings
    dg, db, coef = coefs[2]
    a64 = k.gamma.double() * k.invstd.double()
    assert torch.equal(coef[:C], a64.float())
    k2 = -a64 * dg.double() * k.invstd.double() / k.rows
    B._within(coef[C:2 * C], k2, B.U * 5 * k2.abs(), "k2")
    ka, kb = -a64 * db.double() / k.rows, k2 * k.mean.double()
    B._within(coef[2 * C:], ka - kb, B.U * 9 * (ka.abs() + kb.abs()), "k3")
    assert n == 3
