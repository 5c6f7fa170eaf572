"""GPU: the SegFormer-Lite baseline (the reference's Extended_Baseline_Comparison.py:622-744, BCELoss + Adam :780-837) on the HIP kernels.

  kernels   reduced-KV attention forward / backward, depthwise 3x3 + GELU, BatchNorm + GELU, the NHWC bilinear resize into a channel slice and
            the widened general convolution (7x7 stride 4, kernel = stride = 8 / 4 / 2) against float64 math on the CPU
  model     one train step against the reference goldens (tests/golden/segformer_*), decision-aware gradient parity against the CPU
            restatement (tests/segformer_ref.py), a non-square size, and the 16 x 256^2 benchmark size (determinism, graph capture)
"""
import importlib
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, load_npz

import segformer_ref as fref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PKG = "eusipco-2026-robust-unet_amd"


def _mod(name):
    return importlib.import_module(f"{PKG}.{name}")


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _err(got, want):
    """max |got - want| / max |want|"""
    want = want.double().cpu()
    return float((got.double().cpu() - want).abs().max()) / max(float(want.abs().max()), 1e-30)


def _nhwc_view(t, pad):
    """t [n, h, w, c] -> the same values as a channel slice of a wider [n, h, w, c + pad] buffer (pixel stride c + pad)"""
    n, h, w, c = t.shape
    wide = torch.randn((n, h, w, c + pad), device=DEV)
    wide[..., :c] = t
    return wide[..., :c]


# ------------------------------------------------------------------------------------------------------------ attention
def _attn_ref(q, kv, heads):
    """float64: q [n, nq, C], kv [n, nk, 2C] -> o [n, nq, C], lse [n, heads, nq] (the reference's head split and scale)"""
    n, nq, c = q.shape
    nk = kv.shape[1]
    qh = q.reshape(n, nq, heads, 32).permute(0, 2, 1, 3)
    k = kv[..., :c].reshape(n, nk, heads, 32).permute(0, 2, 1, 3)
    v = kv[..., c:].reshape(n, nk, heads, 32).permute(0, 2, 1, 3)
    s = (qh @ k.transpose(-2, -1)) * 32 ** -0.5
    o = (s.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(n, nq, c)
    return o, torch.logsumexp(s, -1)


@pytest.mark.parametrize("n,heads,nq,nk", [(2, 1, 4096, 64), (2, 2, 1024, 64), (2, 4, 256, 64), (2, 1, 33, 4), (2, 2, 100, 9), (2, 4, 257, 256),
                                           (2, 1, 200, 130), (16, 1, 16384, 64), (16, 1, 8192, 130), (16, 1, 4096, 64)])
def test_kv_attention_matches_float64(pkg, n, heads, nq, nk):
    """o, lse, dq and dkv within 1e-5 of each tensor's largest magnitude, also with a gradient of lse; strided q / kv / dO views; a second
    pass gives the same bits.  The n = 16 cases have more query tiles than blocks per (image, head): forward blocks that walk 4 tiles past
    one staged key tile (16384, 64) or restage 3 key tiles per query tile (8192, 130), backward blocks that add 2 to 8 tiles into their slot."""
    sf = _mod("segformer")
    c = 32 * heads
    g = torch.Generator().manual_seed(nq * 7 + nk)
    q = torch.randn((n, 1, nq, c), generator=g)
    kv = torch.randn((n, 1, nk, 2 * c), generator=g)
    do = torch.randn((n, 1, nq, c), generator=g)
    dlse = torch.randn((n, heads, nq), generator=g) * 0.1
    qd, kvd, dod = _nhwc_view(q.to(DEV), 8), _nhwc_view(kv.to(DEV), 4), _nhwc_view(do.to(DEV), 12)
    o, lse = sf.kv_attention(qd, kvd, heads)
    dq, dkv = sf.kv_attention_backward(qd, kvd, o, lse, dod, heads, dlse=dlse.to(DEV))
    torch.cuda.synchronize()
    q64, kv64 = q.double()[:, 0].requires_grad_(True), kv.double()[:, 0].requires_grad_(True)
    o_ref, lse_ref = _attn_ref(q64, kv64, heads)
    ((o_ref * do.double()[:, 0]).sum() + (lse_ref * dlse.double()).sum()).backward()
    errs = dict(o=_err(o[:, 0], o_ref.detach()), lse=_err(lse, lse_ref.detach()), dq=_err(dq[:, 0], q64.grad), dkv=_err(dkv[:, 0], kv64.grad))
    print(f"\nattention heads {heads} nq {nq} nk {nk}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= 1e-5, errs
    dq2, dkv2 = sf.kv_attention_backward(qd, kvd, o, lse, dod, heads, dlse=dlse.to(DEV))
    o2, lse2 = sf.kv_attention(qd, kvd, heads)
    assert _same(dq, dq2) and _same(dkv, dkv2) and _same(o, o2) and _same(lse, lse2)


# ------------------------------------------------------------------------------------------------------------ depthwise 3x3 + GELU
@pytest.mark.parametrize("n,h,w,c", [(2, 64, 64, 128), (2, 32, 32, 256), (2, 16, 16, 512), (3, 5, 7, 12)])
def test_dwconv_gelu_matches_float64(pkg, n, h, w, c):
    sf = _mod("segformer")
    g = torch.Generator().manual_seed(h * c)
    x = torch.randn((n, h, w, c), generator=g)
    wt = torch.randn((c, 1, 3, 3), generator=g) / 3
    b = torch.randn(c, generator=g) * 0.1
    da = torch.randn((n, h, w, c), generator=g)
    w3 = wt.permute(2, 3, 1, 0).contiguous().to(DEV)                 # [3, 3, 1, c]
    xd = _nhwc_view(x.to(DEV), 4)
    z, a = sf.dwconv_gelu(xd, w3, b.to(DEV))
    dad = da.to(DEV).clone()
    dx, dwdb = sf.dwconv_gelu_backward(xd, z, dad, w3, b.to(DEV))
    # z recomputed in the weight-gradient pass (the model's default): the same arithmetic as the forward, the same bits
    z2, a2 = sf.dwconv_gelu(xd, w3, b.to(DEV), keep_z=False)
    dx2, dwdb2 = sf.dwconv_gelu_backward(xd, None, da.to(DEV).clone(), w3, b.to(DEV))
    torch.cuda.synchronize()
    assert z2 is None and _same(a, a2) and _same(dx, dx2) and _same(dwdb, dwdb2)
    x64 = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    w64, b64 = wt.double().requires_grad_(True), b.double().requires_grad_(True)
    a_ref = F.gelu(F.conv2d(x64, w64, b64, padding=1, groups=c))
    a_ref.backward(da.double().permute(0, 3, 1, 2))
    errs = dict(a=_err(a.permute(0, 3, 1, 2), a_ref.detach()), dx=_err(dx.permute(0, 3, 1, 2), x64.grad),
                dw=_err(dwdb[:9 * c].view(3, 3, c).permute(2, 0, 1), w64.grad[:, 0]), db=_err(dwdb[9 * c:], b64.grad))
    print(f"\ndwconv {n}x{h}x{w}x{c}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= 1e-5, errs


# ------------------------------------------------------------------------------------------------------------ BatchNorm + GELU
@pytest.mark.parametrize("n,h,w,c", [(4, 64, 64, 32), (4, 16, 16, 128), (2, 8, 8, 256), (3, 5, 7, 12)])
def test_bn_gelu_matches_float64(pkg, n, h, w, c):
    sf, B = _mod("segformer"), _mod("blocks")
    g = torch.Generator().manual_seed(c + h)
    t = torch.randn((n, h, w, c), generator=g) * 2 + 0.5
    gamma, beta = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    dy = torch.randn((n, h, w, c), generator=g)
    td = t.to(DEV)
    st = B.BNState(gamma.to(DEV), beta.to(DEV), torch.zeros(c, device=DEV), torch.ones(c, device=DEV), torch.zeros((), dtype=torch.int64, device=DEV))
    s, sh, mean, invstd, _ = B.bn_coeff(td, st, True, B.Small(td.device))
    y = sf.bn_apply_gelu(td, s, sh)
    sums = torch.empty(2 * c, device=DEV)
    dx = sf.bn_backward_gelu(dy.to(DEV), td, mean, invstd, s, sums, sh, training=True)
    torch.cuda.synchronize()
    t64 = t.double().permute(0, 3, 1, 2).requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y_ref = F.gelu(F.batch_norm(t64, None, None, g64, b64, True, 0.0, 1e-5))
    y_ref.backward(dy.double().permute(0, 3, 1, 2))
    errs = dict(y=_err(y.permute(0, 3, 1, 2), y_ref.detach()), dx=_err(dx.permute(0, 3, 1, 2), t64.grad), dgamma=_err(sums[:c], g64.grad),
                dbeta=_err(sums[c:], b64.grad))
    print(f"\nbn+gelu {n}x{h}x{w}x{c}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= 1e-5, errs


# ------------------------------------------------------------------------------------------------------------ NHWC bilinear into a slice
@pytest.mark.parametrize("h,w,ho,wo", [(8, 8, 64, 64), (16, 16, 64, 64), (32, 32, 64, 64), (5, 7, 24, 20)])
def test_bilinear_nhwc_slice_matches_interpolate(pkg, h, w, ho, wo):
    sf = _mod("segformer")
    n, c = 2, 256
    g = torch.Generator().manual_seed(h * 100 + w)
    x = torch.randn((n, h, w, c), generator=g)
    wide = torch.randn((n, ho, wo, 1024), generator=g).to(DEV)
    keep = wide.clone()
    sf.bilinear_nhwc(x.to(DEV), wide[..., 256:512])
    dwide = torch.randn((n, ho, wo, 1024), generator=g)
    dx = sf.bilinear_nhwc_backward(dwide.to(DEV)[..., 512:768], h, w)
    torch.cuda.synchronize()
    x64 = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    y_ref = F.interpolate(x64, size=(ho, wo), mode="bilinear", align_corners=False)
    y_ref.backward(dwide[..., 512:768].double().permute(0, 3, 1, 2))
    errs = dict(y=_err(wide[..., 256:512].permute(0, 3, 1, 2), y_ref.detach()), dx=_err(dx.permute(0, 3, 1, 2), x64.grad))
    assert max(errs.values()) <= 1e-5, errs
    assert torch.equal(wide[..., :256], keep[..., :256]) and torch.equal(wide[..., 512:], keep[..., 512:])


# ------------------------------------------------------------------------------------------------------------ widened general convolution
@pytest.mark.parametrize("cin,cout,k,stride,pad,size", [(3, 32, 7, 4, 3, 64), (32, 32, 8, 8, 0, 64), (64, 64, 4, 4, 0, 32), (128, 128, 2, 2, 0, 16)])
def test_widened_general_conv_matches_float64(pkg, cin, cout, k, stride, pad, size):
    """forward, data gradient (not for the RGB stem) and weight gradient of patch_embed1 (cin 3 padded to 4) and the key / value reductions
    (kernel = stride, no padding) within 1e-5 of scale"""
    ops, B = _mod("ops"), _mod("blocks")
    n = 2
    g = torch.Generator().manual_seed(k * 10 + stride)
    x = torch.randn((n, cin, size, size), generator=g)
    wt = torch.randn((cout, cin, k, k), generator=g) / np.sqrt(cin * k * k)
    b = torch.randn(cout, generator=g) * 0.1
    x64 = x.double().requires_grad_(True)
    w64 = wt.double().requires_grad_(True)
    y_ref = F.conv2d(x64, w64, b.double(), stride=stride, padding=pad)
    dy = torch.randn(y_ref.shape, generator=g)
    y_ref.backward(dy.double())
    xd = B.to_nhwc_pad(x.to(DEV), 4) if cin == 3 else x.to(DEV).permute(0, 2, 3, 1).contiguous()
    wd = wt.permute(2, 3, 1, 0).contiguous().to(DEV)
    y = ops.conv_general_fwd(xd, wd, b.to(DEV), stride, pad)
    dyd = dy.to(DEV).permute(0, 2, 3, 1).contiguous()
    dw = ops.conv_general_wgrad(xd, dyd, k, k, stride, pad, cin_w=cin)
    errs = dict(y=_err(y.permute(0, 3, 1, 2), y_ref.detach()), dw=_err(dw.permute(3, 2, 0, 1), w64.grad))
    if cin != 3:
        dx = ops.conv_general_dgrad(dyd, wd, size, size, stride, pad)
        errs["dx"] = _err(dx.permute(0, 3, 1, 2), x64.grad)
    torch.cuda.synchronize()
    print(f"\nconv {cin}->{cout} k{k} s{stride} p{pad} at {size}^2: " + " ".join(f"{kk} {v:.1e}" for kk, v in errs.items()))
    assert max(errs.values()) <= 1e-5, errs


# ------------------------------------------------------------------------------------------------------------ custom ops
def test_segformer_custom_ops(pkg):
    """runet::kv_attention_nhwc and runet::dwconv3x3_gelu_nhwc: torch.library.opcheck (schema, fake tensor, autograd registration), and their
    autograd equals the direct calls bit for bit (both outputs of the attention carry a gradient)"""
    sf = _mod("segformer")
    importlib.import_module(PKG + ".custom_ops")
    g = torch.Generator().manual_seed(5)
    heads, c = 2, 64
    q = torch.randn((2, 12, 20, c), generator=g).to(DEV)
    kv = torch.randn((2, 3, 5, 2 * c), generator=g).to(DEV)
    do, dlse = torch.randn((2, 12, 20, c), generator=g).to(DEV), torch.randn((2, heads, 240), generator=g).to(DEV)
    qg, kvg = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
    o, lse = torch.ops.runet.kv_attention_nhwc(qg, kvg, heads)
    torch.autograd.backward((o, lse), (do, dlse))
    o_d, lse_d = sf.kv_attention(q, kv, heads)
    dq_d, dkv_d = sf.kv_attention_backward(q, kv, o_d, lse_d, do, heads, dlse=dlse)
    assert _same(o, o_d) and _same(lse, lse_d) and _same(qg.grad, dq_d) and _same(kvg.grad, dkv_d)
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    torch.library.opcheck(torch.ops.runet.kv_attention_nhwc.default, (qg, kvg, heads), test_utils=utils)
    torch.library.opcheck(torch.ops.runet.kv_attention_nhwc_bwd.default, (q, kv, o_d, lse_d, do, dlse, heads), test_utils=("test_schema", "test_faketensor"))
    x = torch.randn((2, 9, 11, 16), generator=g).to(DEV)
    w3 = (torch.randn((3, 3, 1, 16), generator=g) / 3).to(DEV)
    b = (torch.randn(16, generator=g) * 0.1).to(DEV)
    da = torch.randn((2, 9, 11, 16), generator=g).to(DEV)
    xg, wg, bg = x.clone().requires_grad_(True), w3.clone().requires_grad_(True), b.clone().requires_grad_(True)
    a = torch.ops.runet.dwconv3x3_gelu_nhwc(xg, wg, bg)
    a.backward(da)
    _, a_d = sf.dwconv_gelu(x, w3, b, keep_z=False)
    dx_d, dwdb_d = sf.dwconv_gelu_backward(x, None, da.clone(), w3, b)
    assert _same(a, a_d) and _same(xg.grad, dx_d) and _same(wg.grad.reshape(-1), dwdb_d[:9 * 16]) and _same(bg.grad, dwdb_d[9 * 16:])
    torch.library.opcheck(torch.ops.runet.dwconv3x3_gelu_nhwc.default, (xg, wg, bg), test_utils=utils)
    torch.library.opcheck(torch.ops.runet.dwconv3x3_gelu_nhwc_bwd.default, (x, w3, b, da), test_utils=("test_schema", "test_faketensor"))


# ------------------------------------------------------------------------------------------------------------ model
def _zero_mask(k, numel):
    m = np.zeros(numel, dtype=bool)
    if k in fref.ZERO_GRAD:
        m[:] = True
    elif k.endswith(".kv.bias"):
        m[:numel // 2] = True
    return m


def _net(pkg, st):
    net = pkg.SegFormerLite()
    res = net.load_state_dict(st, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return net.to(DEV).train()


def _pick(gold, key, t):
    t = t.detach().cpu().double().reshape(-1)
    if key in gold:
        return t.float().numpy(), gold[key].reshape(-1)
    stride, numel, k = (int(v) for v in gold[key + "/meta"])
    assert t.numel() == numel
    return t[::stride][:k].float().numpy(), gold[key + "/sample"]


@pytest.mark.parametrize("tag", ["n2_s64", "n2_s256"])
def test_segformer_train_step_matches_reference(pkg, tag):
    """test_gpu_segnet.py's bands; the analytically zero gradients (segformer_ref.ZERO_GRAD and the key half of attn*.kv.bias) within 1e-4 of
    the largest gradient norm, absolute."""
    meta = json.load(open(os.path.join(GOLDEN, f"segformer_{tag}.json")))
    gold = load_npz(f"segformer_{tag}.npz")
    st = fref.init_state(seed=meta["seed"], perturb_bn=True)
    net = _net(pkg, st)
    x, y = pkg.synthetic_batch(meta["n"], meta["size"], seed=meta["seed"])
    opt = pkg.FusedAdam(net.parameters(), lr=1e-4, weight_decay=1e-4)
    opt.zero_grad()
    prob = net(x.to(DEV))
    loss = pkg.bce_loss(prob, y.to(DEV))
    loss.backward()
    a, b = _pick(gold, "prob", prob)
    assert np.abs(a - b).max() <= 1e-3, np.abs(a - b).max()
    assert abs(loss.item() - float(gold["loss"])) <= 1e-4
    names = meta["param_names"]
    assert [k for k, _ in net.named_parameters()] == names
    gn = np.array([p.grad.double().norm().item() for p in net.parameters()])
    ref = gold["grad_norm"]
    real = np.array([k not in fref.ZERO_GRAD for k in names])
    rel = np.abs(gn - ref) / (ref + 1e-3 * ref.max())
    assert rel[real].max() < 2e-2, (names[int(np.argmax(np.where(real, rel, 0)))], rel[real].max())
    gmax = max(float(np.abs(v).max()) for kk, v in gold.items() if kk.startswith("grad/") and not kk.endswith("/meta"))
    for k, p in net.named_parameters():
        a, b = _pick(gold, "grad/" + k, p.grad)
        z = _zero_mask(k, p.numel()) if a.size == p.numel() else np.zeros(a.size, dtype=bool)
        if z.any():
            assert np.abs(a[z]).max() <= 1e-4 * ref.max() and np.abs(b[z]).max() <= 1e-4 * ref.max(), (k, np.abs(a[z]).max())
        if not (~z).any():
            continue
        a, b = a[~z], b[~z]
        scale = max(float(np.abs(b).max()), 1e-3 * gmax)
        err = np.abs(a - b)
        assert err.max() <= 0.2 * scale and int((err > 3e-2 * scale).sum()) <= max(1, err.size // 100), (k, err.max(), scale)
        assert float(np.linalg.norm(a - b)) <= 1e-2 * scale * np.sqrt(err.size), (k, float(np.linalg.norm(a - b)), scale)
    for k, buf in net.named_buffers():
        if f"buf/{k}" in gold:
            np.testing.assert_allclose(buf.cpu().numpy(), gold[f"buf/{k}"], rtol=2e-3, atol=2e-3, err_msg=k)
    opt.step()
    for k, p in net.named_parameters():
        a, b = _pick(gold, "adam/" + k, p)
        assert np.abs(a - b).max() <= 2.1e-4, (k, np.abs(a - b).max())         # one Adam step moves each weight by at most lr
    net.eval()
    with torch.no_grad():
        pe = net(x.to(DEV))
    a, b = _pick(gold, "eval_prob", pe)
    assert np.abs(a - b).max() <= 2e-3, np.abs(a - b).max()


def _record_decisions(monkeypatch):
    """Wraps segformer.segformer_backward: the step's two ReLU masks (linear_fuse, head) in the restatement's call order, from the saved
    BatchNorm input and coefficients with bn_apply's own arithmetic"""
    B = _mod("blocks")
    sf = _mod("segformer")
    got = {}
    real = sf.segformer_backward

    def spy(net_, C, dprob):
        got["dec"] = [(B.bn_apply(C[k]["t"], C[k]["s"], C[k]["h"], None, relu=True) > 0).permute(0, 3, 1, 2).cpu() for k in ("fuse", "head")]
        return real(net_, C, dprob)

    monkeypatch.setattr(sf, "segformer_backward", spy)
    return got


def _oracle(st, x, y, forced=None):
    import decisions_seq as DS
    names = fref.param_names()
    P = {k: v.clone() for k, v in st.items()}
    for k in names:
        P[k].requires_grad_(True)
    out = {}

    def step(rec):
        out["p"] = fref.forward(P, x, True)
        return (lambda q: out.setdefault("loss", fref.bce_mean(q, y))), out["p"], None
    log, pr = DS.run_oracle(fref, step, forced)
    return log, {k: P[k].grad for k in names}, pr


@pytest.mark.parametrize("n,size,seed", [(2, 64, 5), (2, 256, 6)])
def test_segformer_gradients_under_the_hip_decisions(pkg, n, size, seed, monkeypatch):
    """tests/decisions_seq.py's two-part check: ReLU masks on which the HIP step and the restatement differ are near-ties, and under the HIP
    step's own masks every gradient (but the analytically zero ones) is within 5e-4 of its tensor's scale, median within 3e-5."""
    import decisions_seq as DS
    st = fref.init_state(seed=seed, perturb_bn=True)
    net = _net(pkg, st)
    x, y = pkg.synthetic_batch(n, size, seed=seed)
    got = _record_decisions(monkeypatch)
    prob = net(x.to(DEV))
    pkg.bce_loss(prob, y.to(DEV)).backward()
    torch.cuda.synchronize()
    log, _, ref_prob = _oracle(st, x, y)
    assert float((prob.detach().cpu() - ref_prob).abs().max()) <= 1e-3
    flips = DS.differing(got["dec"], log)
    DS.assert_near_ties(flips)
    _, gref, _ = _oracle(st, x, y, got["dec"])
    rows = DS.grad_errors({k: p.grad.detach().cpu() for k, p in net.named_parameters()}, gref, set(fref.ZERO_GRAD))
    med = float(np.median([r[0] for r in rows]))
    print(f"\nSegFormerLite {n} x {size}^2: {len(flips)} near-tie decisions forced; worst gradient errors / scale "
          f"{[(f'{e:.1e}', k) for e, k in rows[:4]]}, median {med:.1e}")
    assert rows[0][0] <= 5e-4, rows[:4]
    assert med <= 3e-5, med


def test_segformer_non_square_forward_and_size_bound(pkg):
    """2 x 3 x 96 x 160 (attention Nk = 15 at every stage) against the restatement; a size that is not a multiple of 32 is refused"""
    st = fref.init_state(seed=9, perturb_bn=True)
    net = _net(pkg, st)
    x, _ = pkg.synthetic_batch(2, 160, seed=9)
    x = x[:, :, :96, :].contiguous()
    with torch.no_grad():
        got = net(x.to(DEV)).cpu()
        want = fref.forward({k: v.clone() for k, v in st.items()}, x, True)
    assert got.shape == (2, 1, 96, 160)
    assert float((got - want).abs().max()) <= 1e-3, float((got - want).abs().max())
    with pytest.raises(ValueError):
        net(torch.zeros((1, 3, 96, 80), device=DEV))
    with pytest.raises(ValueError):
        net(torch.zeros((1, 3, 48, 64), device=DEV))


def test_segformer_benchmark_size_is_deterministic_and_captures(pkg):
    """16 x 256^2: finite loss; two steps from an identical state give identical bits; TrainStep(graph=True) replay == eager, bit for bit, with
    p.grad at fixed addresses."""
    trainer = _mod("trainer")
    st = fref.init_state(seed=3, perturb_bn=True)
    x, y = pkg.synthetic_batch(16, 256, seed=31)
    x, y = x.to(DEV), y.to(DEV)
    runs = []
    for _ in range(2):
        net = _net(pkg, st)
        loss = pkg.bce_loss(net(x), y)
        loss.backward()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss))
        runs.append((loss.detach().clone(), [p.grad.detach().clone() for p in net.parameters()], [b.detach().clone() for b in net.buffers()]))
        del net
    assert _same(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1] + runs[0][2], runs[1][1] + runs[1][2]):
        assert torch.equal(a, b)
    del runs
    res = {}
    for graph in (False, True):
        net = _net(pkg, st)
        step = trainer.TrainStep(net, lr=1e-3, weight_decay=1e-4, graph=graph)
        step.optimizer.capturable = True
        ptrs, losses = [], []
        for i in range(5):
            xi, yi = pkg.synthetic_batch(16, 256, seed=80 + i)
            losses.append(step(xi.to(DEV), yi.to(DEV)).detach().clone())
            ptrs.append([p.grad.data_ptr() for p in net.parameters()])
        torch.cuda.synchronize()
        if graph:
            assert step._graph is not None
        else:
            assert all(a == ptrs[0] for a in ptrs[1:]), "p.grad moved between eager steps"
        res[graph] = (losses, [p.detach().clone() for p in net.parameters()], [b.detach().clone() for b in net.buffers()])
        del step, net
    for a, b in zip(res[False][0], res[True][0]):
        assert torch.equal(a, b), (float(a), float(b))
    for a, b in zip(res[False][1] + res[False][2], res[True][1] + res[True][2]):
        assert torch.equal(a, b)


def test_segformer_trains_under_model_evaluator(pkg):
    """ModelEvaluator.train_model / evaluate_model drive SegFormerLite unchanged for 2 epochs; the eval-mode forward of the trained weights
    equals the restatement on the same state."""
    net = _net(pkg, fref.init_state(seed=1))
    ev = pkg.ModelEvaluator(torch.device(DEV))
    x, y = pkg.synthetic_batch(4, 64, seed=2)
    data = [(x[:2], y[:2]), (x[2:], y[2:])]
    out = ev.train_model(net, data, data, epochs=2, lr=1e-3)
    assert len(out["history"]["train_loss"]) == 2 and all(np.isfinite(out["history"]["val_loss"]))
    res = ev.evaluate_model(net, data)
    assert res["total_samples"] == 4 and 0.0 <= res["mean_iou"] <= 1.0
    st = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        got = net(x.to(DEV)).cpu()
        want = fref.forward(st, x, training=False)
    assert float((got - want).abs().max()) <= 1e-3
