"""No GPU: the float64 reference that tests/test_gpu_qtrain_edges.py compares the training query side with, pinned to
`oracle/poly_oracle.update_stage`, and every condition that file's cases rely on, computed from the seeds
(tests/qtrain_edge_cases.py).

  * `query_side` fed the exact pooled sums and pixel counts of real maps reproduces `update_stage`'s cls, obj, dobj, kmask W_t,
    kdep W_d and, through them, its mask and depth maps, <= 1e-12 in float64, values and autograd gradients;
  * the value fixtures reach what they are named for: scores beyond +-100 (`sharp`), sigmoid arguments beyond +-100 (`gates`),
    row mean / spread >= 100 at every LayerNorm behind a raised bias (`offset`), every pixel count of {0, 1, 37, 32768}
    (`counts`), gains of both signs and exact zeros (`norms`);
  * of every case: the float32 run is finite, takes the side of the float64 run at every ReLU, and no float64 ReLU input lies
    within the margin of 0;  S1's float64 gradient of the q and k rows of in_proj is exactly 0;  the two runs take under a second."""
import time

import pytest
import torch

import helpers as Hh
import qtrain_edge_cases as QC
from oracle import poly_oracle as O


def test_cases_need_no_library(monkeypatch):
    """building the head whose shapes the cases take, a case and its two runs never asks for libpolyhead.so (past the caches)"""
    from polyphonicformer_amd import _lib
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("a case asked for libpolyhead.so"))
    assert len(QC._shipped_shapes.__wrapped__()) == 83
    c = QC.case.__wrapped__("S2")
    assert len(QC.run(c["sd"], c["inp"], c["cot"], torch.float32)) == 90


def test_query_side_reproduces_update_stage():
    B, N, L, Fd, H, W = 2, 5, 19, 256, 6, 7
    sd = {n: v.double() for n, v in QC.state(L, Fd, 901).items()}
    g = QC.gen(902)
    x, dfe = torch.randn(B, 256, H, W, generator=g).double(), torch.randn(B, 256, H, W, generator=g).double()
    k, q = torch.randn(B, N, 256, generator=g).double(), torch.randn(B, N, 256, generator=g).double()
    m = torch.randn(B, N, H, W, generator=g).double() - 0.3
    cot = {n: torch.randn(s, generator=g).double() for n, s in
           (("cls", (B, N, L)), ("mask", (B, N, H, W)), ("obj", (B, N, 256)), ("depth", (B, N, H, W)), ("dobj", (B, N, 256)))}
    M = O.binarize(m).double()
    cnt = M.flatten(2).sum(-1)
    assert 0 < float(cnt.min()) and float(cnt.max()) < H * W
    names = sorted(sd)

    def grads(fn):
        with torch.enable_grad():
            w = {n: sd[n].clone().requires_grad_(True) for n in names}
            leaves = [t.clone().requires_grad_(True) for t in (x, dfe, k, q)]
            r = fn(w, *leaves)
            gr = torch.autograd.grad(sum((r[n] * cot[n]).sum() for n in cot), leaves + [w[n] for n in names])
        return {n: v.detach() for n, v in r.items()}, gr

    def staged(w, x_, dfe_, k_, q_):
        return O.update_stage(w, "", x_, k_, m, q_, dfe_, hard_mask=M)

    def folded(w, x_, dfe_, k_, q_):
        pooled = torch.stack([torch.einsum("bnhw,bchw->bnc", M, x_), torch.einsum("bnhw,bchw->bnc", M, dfe_)])
        cls, kern, kbias, obj = QC.query_side(w, pooled, cnt, k_, q_)
        return dict(cls=cls, obj=obj[0], dobj=obj[1], kern=kern[0], kern_d=kern[1],
                    mask=torch.einsum("bnc,bchw->bnhw", kern[0], x_) + kbias[0][..., None, None],
                    depth=torch.einsum("bnc,bchw->bnhw", kern[1], dfe_) + kbias[1][..., None, None])

    r, gr = grads(staged)
    f, gf = grads(folded)
    r["kern"] = r["kmask"] @ sd["feat_transform.conv.weight"].flatten(1)
    r["kern_d"] = r["kdep"] @ sd["feat_depth_transform.conv.weight"].flatten(1)
    err = {n: Hh.rel_err(f[n], r[n]) for n in ("cls", "obj", "dobj", "kern", "kern_d", "mask", "depth")}
    gerr = max(Hh.rel_err(a, b) for a, b in zip(gf, gr))
    print(err, "gradients", gerr)
    assert max(err.values()) <= 1e-12 and gerr <= 1e-12


def test_norms_fixture_has_gains_of_both_signs_and_zeros():
    sd = QC.case("norms")["sd"]
    gains = QC.ln_gains(sd)
    assert len(gains) == 2 * 8 + 1                   # per branch: 5 of the updator, attention_norm, ffn_norm, tower 0; cls_fcs.1
    allg = torch.cat([sd[n] for n in gains])
    zeros = float((allg == 0).float().mean())
    print("norms: zero gains", zeros, "range", float(allg.min()), float(allg.max()))
    for n in gains:
        assert (sd[n] > 0).any() and (sd[n] < 0).any() and (sd[n] == 0).any() and float(sd[n].abs().max()) <= 4.0, n
    assert 0.03 < zeros < 0.07
    biases = torch.cat([v for n, v in sd.items() if v.dim() == 1 and n.endswith(".bias")])
    assert 0.9 < float(biases.std()) < 1.1


def test_sharp_fixture_scores_pass_100():
    c = QC.case("sharp")
    rng = QC.score_range(c["sd"], c["inp"])
    print("sharp: factor", c["factor"], "score range per branch", rng)
    assert all(hi > 100.0 and lo < -100.0 for hi, lo in rng)
    assert all(hi < 20.0 for hi, lo in QC.score_range(QC.case("S4")["sd"], QC.case("S4")["inp"]))       # a plain case does not


def test_gates_fixture_saturates_the_sigmoids():
    c = QC.case("gates")
    t = QC.trace(c["sd"], c["inp"])
    for s in ("", "_depth"):
        for n in QC.GATE_NORMS:
            a = t["ln_out"][n.format(s=s)]
            print("gates:", n.format(s=s), "largest |argument|", float(a.abs().max()))
            assert float(a.max()) > 100.0 and float(a.min()) < -100.0
            sg = a.float().sigmoid()
            dead = a.abs() > 100.0
            assert (sg[dead] * (1.0 - sg[dead]) == 0).all()             # s (1 - s) is exactly 0 there in float32


def test_offset_fixture_rows_sit_far_from_zero():
    c = QC.case("offset")
    t = QC.trace(c["sd"], c["inp"])
    for s in ("", "_depth"):
        for n in QC.OFFSET_NORMS:
            x = t["ln_in"][n.format(s=s)]
            ratio = x.mean(-1).abs() / x.std(-1, unbiased=False)
            print("offset:", n.format(s=s), "least |mean| / spread", float(ratio.min()))
            assert float(ratio.min()) >= 100.0


def test_counts_fixture_has_every_count():
    inp = QC.case("counts")["inp"]
    for v in QC.COUNT_VALUES:
        assert int((inp["cnt"] == v).sum()) >= 1, v
    empty = inp["cnt"] == 0
    assert (inp["pooled"][:, empty] == 0).all() and (inp["pooled"][:, ~empty].abs().amax(-1) > 0).all()


@pytest.mark.parametrize("name", QC.CASES)
def test_case_conditions(name):
    c = QC.case(name)
    B, N, L, Fd = c["shape"]
    assert c["inp"]["pooled"].shape == (2, B, N, 256) and c["cot"]["cls"].shape == (B, N, L)
    assert c["sd"]["ffn.layers.0.0.weight"].shape == (Fd, 256) and c["sd"]["fc_cls.weight"].shape == (L, 256)
    t0 = time.perf_counter()
    r64 = QC.run(c["sd"], c["inp"], c["cot"], torch.float64)
    r32 = QC.run(c["sd"], c["inp"], c["cot"], torch.float32)
    dt = time.perf_counter() - t0
    assert len(r64) == 90 and set(r64) == set(r32)
    for n, v in r32.items():
        assert v.dtype == torch.float32 and v.shape == r64[n].shape and torch.isfinite(v).all(), n
        assert torch.isfinite(r64[n]).all(), n
    e = {n: Hh.rel_err(r32[n], r64[n]) for n in r64 if float(r64[n].abs().max()) > 0}
    worst = max(e, key=e.get)
    print(f"{name}: {dt:.2f} s, {c['rounds']} conditioning rounds, worst e_ref {e[worst]:.2e} ({worst})")
    t64, t32 = QC.trace(c["sd"], c["inp"]), QC.trace(c["sd"], c["inp"], torch.float32)
    for a, b, bias in zip(t64["relu"], t32["relu"], QC.RELU_BIAS):
        assert float(a.abs().min()) >= QC.MARGIN, bias
        assert ((a > 0) == (b > 0)).all(), bias
    assert dt < 1.0


def test_s1_has_no_gradient_into_q_and_k():
    """one key: the softmax is 1 whatever the score, so q and k get no gradient -- exactly, in float64 and on the device"""
    r64, _ = QC.reference("S1")
    for s in ("", "_depth"):
        gw, gb = r64[f"attention{s}.attn.in_proj_weight"], r64[f"attention{s}.attn.in_proj_bias"]
        assert (gw[:512] == 0).all() and (gb[:512] == 0).all()
        assert float(gw[512:].abs().max()) > 1.0 and float(gb[512:].abs().max()) > 1.0
