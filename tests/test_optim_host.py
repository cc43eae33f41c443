"""CPU: the host side of the optimizer step (polyphonicformer_amd/optim.py) -- the work-item plan as a pure function of sizes and
alignments, and the state exchange with `torch.optim.AdamW` in both directions.  No kernel runs; the header and the ctypes mirrors
of the new structs and entry points are covered by tests/test_abi.py."""
import pytest
import torch

from polyphonicformer_amd import optim as O

CHUNK = O.CHUNK


def test_chunk_is_the_headers():
    from polyphonicformer_amd import _lib
    assert CHUNK == _lib.PH_OPTIM_CHUNK == 4096


def test_plan_sizes_around_the_chunk():
    numels = [0, 1, 3, 4095, 4096, 4097, 8197]
    items, first, kinds = O.plan_items(numels, [True] * len(numels))
    assert [(n + CHUNK - 1) // CHUNK for n in numels] == [0, 1, 1, 1, 1, 2, 3]
    assert first == [0, 0, 1, 2, 3, 4, 6] and items == 9
    assert kinds == [None] + ["vec"] * 6
    # every item belongs to the tensor whose range holds it; the tensor without elements owns none (its successor wins the shared number)
    owner = [O.item_tensor(first, i) for i in range(items)]
    assert owner == [1, 2, 3, 4, 5, 5, 6, 6, 6]


def test_plan_offset_by_one_float_is_scalar():
    """a view one float into its storage is 4-byte aligned only: the whole tensor takes the scalar path, the numbering is unchanged"""
    base = torch.zeros(4096 + 4 + 4097 + 1)
    whole, view = base[:4096], base[4096 + 4 + 1:]
    assert view.data_ptr() - whole.data_ptr() == 4 * (4096 + 5) and view.numel() == 4097
    a0 = whole.data_ptr() % 16                                   # whatever the allocator gave: the two differ by one float mod 16
    aligned = [O.all_aligned(t.data_ptr() - a0, 0, 16, 32) for t in (whole, view)]
    assert aligned == [True, False]
    assert not O.all_aligned(0, 16, 32, 4) and not O.all_aligned(8, 0, 0, 0)
    items, first, kinds = O.plan_items([4096, 4097], aligned)
    assert (items, first, kinds) == (3, [0, 1], ["vec", "scalar"])


def test_plan_numbering_across_300_tensors():
    gen = torch.Generator().manual_seed(5)
    numels = torch.randint(0, 3 * CHUNK, (300,), generator=gen).tolist()
    numels[17] = numels[18] = 0                                  # two empty neighbours
    numels[299] = 0                                              # and an empty last tensor: it owns no item
    items, first, _ = O.plan_items(numels, [True] * 300)
    assert items == sum((n + CHUNK - 1) // CHUNK for n in numels)
    want = [t for t, n in enumerate(numels) for _ in range((n + CHUNK - 1) // CHUNK)]
    assert [O.item_tensor(first, i) for i in range(items)] == want
    assert all(b - a == (n + CHUNK - 1) // CHUNK for a, b, n in zip(first, first[1:] + [items], numels))


def test_plan_refuses_a_negative_size():
    with pytest.raises(ValueError):
        O.plan_items([4, -1], [True, True])


# ---- the state exchange --------------------------------------------------------------------------------------------------------------
SHAPES = [(5,), (3, 4), (1,), (7, 2)]


def _params(seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=gen)) for s in SHAPES]


def _groups(ps):
    return [dict(params=ps[:2], lr=1e-2, weight_decay=0.05), dict(params=ps[2:], lr=3e-3, weight_decay=0.0)]


def _stepped_torch(ps, steps=2):
    opt = torch.optim.AdamW(_groups(ps), betas=(0.8, 0.95), eps=1e-7, foreach=False)
    gen = torch.Generator().manual_seed(11)
    for _ in range(steps):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=gen)
        opt.step()
    return opt


def test_state_dict_layout_is_torchs():
    ps = _params(1)
    ours = O.AdamWStep(_groups(ps), lr=1.0, betas=(0.8, 0.95), eps=1e-7, weight_decay=0.5)
    ref = _stepped_torch(_params(1)).state_dict()
    ours.load_state_dict(ref)
    sd = ours.state_dict()
    assert set(sd) == set(ref) == {"state", "param_groups"}
    assert set(sd["state"]) == set(ref["state"]) == {0, 1, 2, 3}
    for i in range(4):
        assert set(sd["state"][i]) == set(ref["state"][i]) == {"step", "exp_avg", "exp_avg_sq"}
        assert float(sd["state"][i]["step"]) == 2.0
        assert torch.equal(sd["state"][i]["exp_avg"], ref["state"][i]["exp_avg"])
        assert torch.equal(sd["state"][i]["exp_avg_sq"], ref["state"][i]["exp_avg_sq"])
    for a, b in zip(sd["param_groups"], ref["param_groups"]):
        assert set(a) == set(b)
        assert {k: a[k] for k in ("lr", "weight_decay", "eps", "params", "amsgrad", "maximize")} == \
            {k: b[k] for k in ("lr", "weight_decay", "eps", "params", "amsgrad", "maximize")}
        assert tuple(a["betas"]) == tuple(b["betas"])
    # the group values of the file replaced the constructor's
    assert [(g["lr"], g["weight_decay"]) for g in ours.param_groups] == [(1e-2, 0.05), (3e-3, 0.0)]


def test_torch_loads_what_we_export():
    ps = _params(2)
    ref = _stepped_torch(ps, steps=3)
    ours = O.AdamWStep(_groups(ps), betas=(0.8, 0.95), eps=1e-7)
    ours.load_state_dict(ref.state_dict())
    assert ours.info()["step"] == 3
    fresh = torch.optim.AdamW(_groups(ps), betas=(0.8, 0.95), eps=1e-7, foreach=False)
    fresh.load_state_dict(ours.state_dict())
    # the same next step from the reloaded state as from the original
    twin = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    ref2 = torch.optim.AdamW(_groups(twin), betas=(0.8, 0.95), eps=1e-7, foreach=False)
    ref2.load_state_dict(ref.state_dict())
    gen = torch.Generator().manual_seed(3)
    for p, q in zip(ps, twin):
        p.grad = torch.randn(p.shape, generator=gen)
        q.grad = p.grad.clone()
    fresh.step()
    ref2.step()
    for p, q in zip(ps, twin):
        assert torch.equal(p, q)
    assert all(float(fresh.state[p]["step"]) == 4.0 for p in ps)


def test_fresh_state_is_empty_as_torchs():
    ps = _params(4)
    ours = O.AdamWStep(ps, lr=1e-3)
    sd = ours.state_dict()
    assert sd["state"] == {} and len(sd["param_groups"]) == 1 and sd["param_groups"][0]["params"] == [0, 1, 2, 3]
    assert sd["param_groups"][0]["weight_decay"] == 1e-2
    torch.optim.AdamW(ps, lr=1e-3).load_state_dict(sd)
    ours.load_state_dict(torch.optim.AdamW(ps, lr=1e-3).state_dict())
    assert ours.info()["step"] == 0


def test_unequal_steps_are_refused_on_import():
    ps = _params(6)
    sd = _stepped_torch(ps).state_dict()
    sd["state"][2]["step"] = torch.tensor(5.0)
    ours = O.AdamWStep(_groups(ps), betas=(0.8, 0.95), eps=1e-7)
    with pytest.raises(ValueError, match="step"):
        ours.load_state_dict(sd)


def test_mismatched_groups_are_refused_on_import():
    ps = _params(6)
    sd = _stepped_torch(ps).state_dict()
    with pytest.raises(ValueError):
        O.AdamWStep(ps, betas=(0.8, 0.95), eps=1e-7).load_state_dict(sd)
    with pytest.raises(ValueError, match="betas"):
        O.AdamWStep(_groups(ps)).load_state_dict(sd)


@pytest.mark.parametrize("kw", [dict(amsgrad=True), dict(maximize=True)])
def test_amsgrad_and_maximize_raise(kw):
    ps = _params(7)
    with pytest.raises(NotImplementedError):
        O.AdamWStep(ps, **kw)
    with pytest.raises(NotImplementedError):
        O.AdamWStep([dict(params=ps, **kw)])
    sd = torch.optim.AdamW(ps, **kw).state_dict()
    with pytest.raises(NotImplementedError):
        O.AdamWStep(ps).load_state_dict(sd)


def test_parameters_are_checked():
    from polyphonicformer_amd import _lib
    with pytest.raises(_lib.PolyheadError, match="fp32"):
        O.AdamWStep([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))])
    with pytest.raises(_lib.PolyheadError, match="contiguous"):
        O.AdamWStep([torch.zeros(4, 6).t().requires_grad_()])
    p = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(ValueError):
        O.AdamWStep([dict(params=[p]), dict(params=[p])])
    p.grad = torch.ones(4)
    with pytest.raises(_lib.PolyheadError, match="GPU"):       # the kernels are the only compute path
        O.AdamWStep([p]).step()
    assert torch.equal(p.detach(), torch.zeros(4))
