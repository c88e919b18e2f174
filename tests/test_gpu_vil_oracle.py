"""-m gpu: the ViL stage (csrc/vil.hip) against the fp64 oracle (oracle.vil_layer, run on the GPU) where the kernels can go
wrong without test_gpu_vil.py noticing:
 (a) long sequences, backward included, on the chunk-recurrent and the tiled path: S = 8192 (the last size whose gate scans
     keep a lane's tokens in registers), 8193 (the first that does not; lanes past 910 own no token), 9000 (not a multiple
     of the 64-token chunk); dx and all 14 parameter gradients against the oracle's autograd,
 (b) the error as a function of token position at S = 32 768: the gate stabilisers F = cumsum(logsigmoid(f)) grow linearly
     with the position, so a stabiliser kept in fp32 loses digits towards the end of the sequence,
 (c) gate regimes: denominator always / never on the exp(-m) floor, dominated by its 1e-6 epsilon, saturated and strongly
     forgetting forget gates, per-token gates (the arg-max of the prefix maximum moves inside a chunk),
 (d) bf16 / fp16 storage up to S = 4096, (e) C = 16 (DH = 8, tiled kernels only), (f) the skip input with add_xa = 1.
Errors are measured on the ViL branch (output minus residual), so the residual does not dilute them."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import xlstm_hved_amd as X  # noqa: E402
import xlstm_hved_oracle as O  # noqa: E402

DEV = "cuda"
NAMES = ["vil.norm.weight", "vil.layer.proj_up.weight", "vil.layer.conv1d.conv.weight", "vil.layer.conv1d.conv.bias",
         "vil.layer.q_proj.weight", "vil.layer.k_proj.weight", "vil.layer.v_proj.weight",
         "vil.layer.mlstm_cell.igate.weight", "vil.layer.mlstm_cell.igate.bias", "vil.layer.mlstm_cell.fgate.weight",
         "vil.layer.mlstm_cell.fgate.bias", "vil.layer.mlstm_cell.outnorm.weight", "vil.layer.learnable_skip",
         "vil.layer.proj_down.weight"]
BOUND_F32 = (2e-5, 2e-5)        # fp32 arithmetic: (max-norm, L2) error of each output and gradient against the fp64 oracle
BOUND_FGATE = (4e-3, 3e-3)      # the forget-gate gradients, on the scale of the largest parameter gradient (see _errs)
FGATE = ("vil.layer.mlstm_cell.fgate.weight", "vil.layer.mlstm_cell.fgate.bias")
GATES = ["vil.layer.mlstm_cell.igate.bias", "vil.layer.mlstm_cell.fgate.bias", "vil.layer.mlstm_cell.igate.weight",
         "vil.layer.mlstm_cell.fgate.weight"]


def _layer(c=32, ig_b=(-2.0, -1.0, 0.0, 1.0), fg_b=(-1.0, 1 / 3, 5 / 3, 3.0), gate_std=0.0, q_scale=1.0, seed=0):
    """ViLLayer(c) with per-head gate biases; gate_std > 0 gives the gates per-token weights (the reset zeroes them);
    q_scale scales the query projection (and with it |b_t|)."""
    torch.manual_seed(seed)
    m = X.ViLLayer(c)
    m.apply(X.init_weights)
    with torch.no_grad():
        cell = m.vil.layer.mlstm_cell
        cell.igate.bias.copy_(torch.tensor(ig_b))
        cell.fgate.bias.copy_(torch.tensor(fg_b))
        if gate_std:
            cell.igate.weight.normal_(0.0, gate_std)
            cell.fgate.weight.normal_(0.0, gate_std)
        m.vil.layer.q_proj.weight.mul_(q_scale)
    return m


class _CellProbe:
    """Wraps the oracle's mLSTM cell to record, per call, the largest |gate| and the fraction of (batch, head, token) rows
    whose denominator sits on the exp(-m) floor (|b_t| < exp(-m_t), vision_lstm.py:120-127)."""

    def __init__(self):
        self.floor, self.epsd, self.gmax, self.fmin, self.fmax, self.istd = [], [], [], [], [], []

    def __enter__(self):
        self.par, self.rec = O.mlstm_parallel, O.mlstm_recurrent
        O.mlstm_parallel = self._wrap(self.par)
        O.mlstm_recurrent = self._wrap(self.rec)
        return self

    def __exit__(self, *a):
        O.mlstm_parallel, O.mlstm_recurrent = self.par, self.rec

    def _wrap(self, fn):
        def cell(q, k, v, igate, fgate, eps=1e-6):
            with torch.no_grad():
                self.gmax.append(max(igate.abs().max().item(), fgate.abs().max().item()))
                self.fmin.append(fgate.min().item())
                self.fmax.append(fgate.max().item())
                self.istd.append(igate.std(dim=2).min().item())         # spread over the tokens, smallest head
                if q.shape[2] <= 4096:
                    S, DH = q.shape[2], q.shape[3]
                    csum = torch.cumsum(torch.nn.functional.logsigmoid(fgate), -2)
                    tril = torch.tril(torch.ones(S, S, dtype=torch.bool, device=q.device))
                    logd = torch.where(tril, csum - csum.transpose(-2, -1) + igate.transpose(-2, -1),
                                       torch.tensor(-math.inf, dtype=q.dtype, device=q.device))
                    mrow = logd.max(-1, keepdim=True)[0]
                    b = ((q @ k.transpose(-2, -1)) / math.sqrt(DH) * torch.exp(logd - mrow)).sum(-1, keepdim=True)
                    self.floor.append((b.abs() < torch.exp(-mrow)).double().mean().item())
                    # rows whose denominator max(|b|, exp(-m)) + eps is within 10x of eps alone
                    self.epsd.append((torch.maximum(b.abs(), torch.exp(-mrow)) < 10 * eps).double().mean().item())
            return fn(q, k, v, igate, fgate, eps)
        return cell


def _oracle(m, x, skip=None, wgt=None, recurrent=False):
    """fp64 on the GPU.  Returns (branch, dx, dskip, {param: grad}); branch = output minus the residual(s):
    without skip  vil_layer(x) - x,  with skip  (x + vil_layer(x + skip)) - x - (x + skip)."""
    sd = {"mViL." + k: v.detach().to(DEV, torch.float64).clone().requires_grad_(wgt is not None)
          for k, v in m.state_dict().items()}
    xo = x.to(DEV, torch.float64).clone().requires_grad_(wgt is not None)
    so = skip.to(DEV, torch.float64).clone().requires_grad_(wgt is not None) if skip is not None else None
    u = xo if so is None else xo + so
    with torch.set_grad_enabled(wgt is not None):
        y = O.vil_layer(O.P(sd).sub("mViL"), u, recurrent=recurrent)
        if so is not None:
            y = xo + y
        gx = gs = gp = None
        if wgt is not None:
            (y * wgt.to(DEV, torch.float64)).sum().backward()
            gx, gs = xo.grad, (so.grad if so is not None else None)
            gp = {k: sd["mViL." + k].grad for k in NAMES}
    branch = (y - u - (xo if so is not None else 0)).detach()
    return branch, gx, gs, gp


def _run(m, x, skip=None, wgt=None, tiled=False, dtype=torch.float32):
    """The HIP stage (fp32 parameters, `dtype` storage).  Returns (branch in fp64, dx, dskip, {param: grad})."""
    lib = X._lib.load()
    lib.xh_set_option(2, 8 if tiled else 0)
    try:
        mg = m.to(DEV)
        for p in mg.parameters():
            p.grad = None
        xg = x.to(DEV, dtype).requires_grad_(wgt is not None)
        sg = skip.to(DEV, dtype).requires_grad_(wgt is not None) if skip is not None else None
        y = mg(xg) if sg is None else mg(xg, sg, residual_input=True)
        assert y.dtype == dtype
        gx = gs = gp = None
        if wgt is not None:
            (y.float() * wgt.to(DEV, dtype).float()).sum().backward()
            gx, gs = xg.grad, (sg.grad if sg is not None else None)
            pn = dict(mg.named_parameters())
            gp = {k: pn[k].grad for k in NAMES}
        torch.cuda.synchronize()
        xd = xg.detach().double()
        res = xd if sg is None else 2 * xd + sg.detach().double()
        return y.detach().double() - res, gx, gs, gp
    finally:
        lib.xh_set_option(2, 0)


def _errs(got, ref):
    """{name: (max-norm, L2) error}.  Outputs are judged against their own size.  A parameter gradient is judged against its
    own size or a tenth of the largest parameter gradient, whichever is larger (an input-gate bias whose constant shift
    cancels in the ratio a / b is zero up to round-off).  The forget-gate gradients are judged against the largest parameter
    gradient, as gpu_common.check_grads does: df_t = sigmoid(-f_t) * sum_{t' >= t} (q.dq - k.dk)_t' is a difference of two
    sums over every later token whose fp32 round-off grows with the sequence while df itself stays of the size of the
    couplings that straddle t (tiny under a strongly forgetting gate)."""
    pscale = max([r.abs().max().item() for k, r in ref.items() if k.startswith("vil.")] or [0.0])
    out = {}
    for k, r in ref.items():
        a, b = got[k].detach().double(), r.detach().double().to(got[k].device)
        fl = pscale if k in FGATE else 0.1 * pscale if k.startswith("vil.") else 0.0
        d = a - b
        out[k] = ((d.abs().max() / max(b.abs().max().item(), fl, 1e-30)).item(),
                  (d.norm() / max(b.norm().item(), fl * b.numel() ** 0.5, 1e-30)).item())
    return out


def _fmt(e):
    return " ".join(f"{'.'.join(k.split('.')[-2:])}={a:.1e}/{b:.1e}" for k, (a, b) in e.items())


def _assert_errs(e, bound, what):
    bad = {k: v for k, v in e.items() if v[0] > (BOUND_FGATE if k in FGATE else bound)[0]
           or v[1] > (BOUND_FGATE if k in FGATE else bound)[1]}
    assert not bad, f"{what}: errors (max-norm/L2) over bound: {_fmt(bad)}"


def _shape(S, c=32, b=1):
    for d in range(int(round(S ** (1 / 3))) + 1, 0, -1):           # a (d, h, w) factorisation of S, w fastest
        if S % d == 0:
            r = S // d
            for h in range(int(math.isqrt(r)), 0, -1):
                if r % h == 0:
                    return (b, c, d, h, r // h)
    return (b, c, 1, 1, S)


# ------------------------------------------------------------------------------------------------ (a) long sequences, backward
@pytest.mark.parametrize("S", [8192, 8193, 9000])
def test_long_sequence_backward_vs_fp64_oracle(S):
    m = _layer(seed=S)
    shape = _shape(S)
    g = torch.Generator().manual_seed(S)
    x, wgt = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    y_o, gx_o, _, gp_o = _oracle(m, x, wgt=wgt)
    ref = {"y": y_o, "dx": gx_o, **gp_o}
    errs = {}
    for path in ("chunk", "tiled"):
        y, gx, _, gp = _run(m, x, wgt=wgt, tiled=path == "tiled")
        errs[path] = _errs({"y": y, "dx": gx, **gp}, ref)
        print(f"S={S} {path} (max/L2): {_fmt(errs[path])}")
    for path, e in errs.items():
        _assert_errs(e, BOUND_F32, f"S={S} {path}")
    del ref, y_o, gx_o, gp_o
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ (b) error against position
def test_forward_error_does_not_grow_with_position_at_32768_tokens():
    """Forget biases -3, -1, 2, 12 (|F| at the last token about 1.1e5, 4.3e4, 4.2e3, 0.2) and per-token gates, B = 2.  fp32
    round-off does not depend on the position: the last 1024-token block must be within 3x the first."""
    S, blk = 32768, 1024
    m = _layer(ig_b=(-1.0, 0.0, 0.5, 1.0), fg_b=(-3.0, -1.0, 2.0, 12.0), gate_std=0.3, seed=7)
    x = torch.randn((2, 32, 32, 32, 32), generator=torch.Generator().manual_seed(7))
    y, _, _, _ = _run(m, x)
    with _CellProbe() as pr:
        y_o, _, _, _ = _oracle(m, x, recurrent=True)
    assert pr.gmax[0] <= 30.0, pr.gmax
    d = (y - y_o).abs().amax(dim=(0, 1)).reshape(-1)                    # per token, over batch and channels
    scale = y_o.abs().max().item()
    per = (d.view(S // blk, blk).amax(1) / scale).tolist()
    print("S=32768 per-block max error / max|branch|: first %.2e  last %.2e  worst %.2e  (blocks 0,8,16,24,31: %s)"
          % (per[0], per[-1], max(per), " ".join(f"{per[i]:.1e}" for i in (0, 8, 16, 24, 31))))
    assert max(per) < 1e-4
    assert per[-1] <= 3 * per[0] + 1e-6, f"error grows with position: first block {per[0]:.2e}, last {per[-1]:.2e}"


# ------------------------------------------------------------------------------------------------ (c) gate regimes
REGIMES = {
    "floor_always": dict(ig_b=(-15.0,) * 4),
    "floor_never": dict(ig_b=(15.0,) * 4),
    "fgate_saturated": dict(fg_b=(12.0,) * 4),
    "fgate_forgetting": dict(fg_b=(-6.0,) * 4),
    "per_token_gates": dict(gate_std=0.3),
    "eps_denominator": dict(ig_b=(20.0,) * 4, q_scale=1e-5),
}


@pytest.mark.parametrize("S", [140, 4096])
@pytest.mark.parametrize("regime", sorted(REGIMES))
def test_gate_regimes_vs_fp64_oracle(regime, S):
    m = _layer(seed=11, **REGIMES[regime])
    shape = _shape(S)
    g = torch.Generator().manual_seed(S + 1)
    x, wgt = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    with _CellProbe() as pr:
        y_o, gx_o, _, gp_o = _oracle(m, x, wgt=wgt)
    fl = pr.floor[0]
    print(f"{regime} S={S}: floor fraction {fl:.3f}, eps-dominated {pr.epsd[0]:.3f}, max|gate| {pr.gmax[0]:.1f}, f in [{pr.fmin[0]:.1f}, {pr.fmax[0]:.1f}], "
          f"token std of i >= {pr.istd[0]:.2f}")
    assert pr.gmax[0] <= 30.0
    if regime == "floor_always":
        assert fl == 1.0
    elif regime == "floor_never":
        assert fl <= 0.01
    elif regime == "fgate_saturated":
        assert pr.fmin[0] >= 11.0                   # sigmoid(f) >= 1 - 2e-5 on every token: memory spans the sequence
    elif regime == "eps_denominator":
        assert pr.epsd[0] >= 0.5                    # the 1e-6 of the denominator (and the dm route of the backward) matters
    elif regime == "fgate_forgetting":
        assert pr.fmax[0] <= -5.0                   # sigmoid(f) <= 7e-3: each token mostly forgets the past
    else:
        assert pr.istd[0] >= 0.2                    # the input gate varies from token to token in every head
    ref = {"y": y_o, "dx": gx_o, **{k: gp_o[k] for k in GATES}}
    errs = {}
    for path in ("chunk", "tiled"):
        y, gx, _, gp = _run(m, x, wgt=wgt, tiled=path == "tiled")
        errs[path] = _errs({"y": y, "dx": gx, **{k: gp[k] for k in GATES}}, ref)
        print(f"  {path} (max/L2): {_fmt(errs[path])}")
    for path, e in errs.items():
        _assert_errs(e, BOUND_F32, f"{regime} S={S} {path}")


# ------------------------------------------------------------------------------------------------ (d) 16-bit storage
def _band(got, ref, unit, tol32, scale, mag=None):
    """Pointwise: |got - ref| <= unit * mag + tol32 * scale, mag = |ref| by default -- the storage rounding of the output
    plus fp32 arithmetic.  Returns (ok, the largest |got - ref| in units of that band)."""
    got, ref = got.double(), ref.double().to(got.device)
    mag = ref.abs() if mag is None else mag.double().to(got.device)
    r = ((got - ref).abs() / (unit * mag + tol32 * scale)).max().item()
    return r <= 1.0, r


@pytest.mark.parametrize("S", [30, 140, 4096])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_16bit_storage_vs_fp64_oracle_on_rounded_inputs(dtype, S):
    """Storage is 16-bit, arithmetic fp32 and the parameters fp32: against the fp64 oracle fed the storage-rounded x and
    output weights, the forward output and dx are off by one rounding (2^-8 bf16, 2^-11 fp16, relative, with a margin of 2)
    plus fp32 round-off; the parameter gradients (fp32 accumulators) meet the fp32 bands."""
    unit = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    m = _layer(seed=S + 5, gate_std=0.1)
    shape = _shape(S, b=2)
    g = torch.Generator().manual_seed(S + 2)
    x = torch.randn(shape, generator=g).to(dtype).float()
    wgt = torch.randn(shape, generator=g).to(dtype).float()
    _, gx_o, _, gp_o = _oracle(m, x, wgt=wgt)
    with torch.no_grad():
        y_full = O.vil_layer(O.P({"mViL." + k: v.to(DEV, torch.float64) for k, v in m.state_dict().items()}).sub("mViL"),
                             x.to(DEV, torch.float64))
    y, gx, _, gp = _run(m, x, wgt=wgt, dtype=dtype)
    y = y + x.to(DEV, torch.float64)                                   # the stored output itself
    ok_y, ry = _band(y, y_full, unit, 1e-5, y_full.abs().max().item())
    ok_x, rx = _band(gx, gx_o, unit, 1e-5, gx_o.abs().max().item())
    e = _errs(gp, gp_o)
    print(f"{dtype} S={S}: y {ry:.2e} dx {rx:.2e} (fraction of the band); params (max/L2): {_fmt(e)}")
    assert ok_y and ok_x
    _assert_errs(e, BOUND_F32, f"{dtype} S={S}")


# ------------------------------------------------------------------------------------------------ (e) C = 16
@pytest.mark.parametrize("S", [64, 140, 4096])
def test_c16_vs_fp64_oracle(S):
    m = _layer(c=16, seed=S + 9, gate_std=0.1)
    shape = _shape(S, c=16)
    g = torch.Generator().manual_seed(S + 3)
    x, wgt = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    y_o, gx_o, _, gp_o = _oracle(m, x, wgt=wgt)
    y, gx, _, gp = _run(m, x, wgt=wgt)
    e = _errs({"y": y, "dx": gx, **gp}, {"y": y_o, "dx": gx_o, **gp_o})
    print(f"C=16 S={S} (max/L2): {_fmt(e)}")
    _assert_errs(e, BOUND_F32, f"C=16 S={S}")


# ------------------------------------------------------------------------------------------------ (f) skip input
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_skip_input_residual_vs_fp64_oracle(dtype):
    """out = x + ViLBlock(x + skip) (RA_HVED.py:626): dx = dout + dxin, dskip = dxin."""
    S = 600
    m = _layer(seed=13, gate_std=0.1)
    shape = _shape(S, b=2)
    g = torch.Generator().manual_seed(13)
    x, skip, wgt = (torch.randn(shape, generator=g).to(dtype).float() for _ in range(3))
    y_o, gx_o, gs_o, gp_o = _oracle(m, x, skip, wgt=wgt)
    y, gx, gs, gp = _run(m, x, skip, wgt=wgt, dtype=dtype)
    if dtype == torch.float32:
        e = _errs({"y": y, "dx": gx, "dskip": gs, **gp}, {"y": y_o, "dx": gx_o, "dskip": gs_o, **gp_o})
        print(f"skip f32 (max/L2): {_fmt(e)}")
        _assert_errs(e, BOUND_F32, "skip f32")
        return
    unit = 2.0 ** -8
    xd, sd_ = x.to(DEV, torch.float64), skip.to(DEV, torch.float64)
    out_o = y_o + 2 * xd + sd_
    out = y + 2 * xd + sd_
    ok_y, ry = _band(out, out_o, unit, 1e-5, out_o.abs().max().item())
    # dx = dout + dxin is rounded twice: dxin on its own (|dxin| = |dskip| may exceed |dx|), then the sum
    ok_x, rx = _band(gx, gx_o, unit, 1e-5, gx_o.abs().max().item(), mag=gx_o.abs() + gs_o.abs())
    ok_s, rs = _band(gs, gs_o, unit, 1e-5, gs_o.abs().max().item())
    e = _errs(gp, gp_o)
    print(f"skip bf16: out {ry:.2e} dx {rx:.2e} dskip {rs:.2e} (fraction of the band); params (max/L2): {_fmt(e)}")
    assert ok_y and ok_x and ok_s
    _assert_errs(e, BOUND_F32, "skip bf16")
