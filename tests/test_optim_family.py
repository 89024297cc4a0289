"""The optimiser / criterion choices of the reference's harness beyond AdamW, LAMB and the robust losses:
FusedSGD, FusedAdam, criterion_with_metrics (RobustL1 / RobustL2 / L1 / L2 with mae and rmse in one launch) and the
trainer's `optim=`, `std_loss=`, `only_residual=` and `validate()`.  References are torch.optim / torch.nn.functional
themselves, which is what the harness calls (CGAT/lightning_module.py:131-142, 240-243, 319-327): recorded on the CPU in
tests/golden/optim_family*.npz, live on the GPU, and evaluated in fp64 on the host.  Tolerance: the project's 1e-5
max-norm relative (tests/test_optim.py), on parameters and momentum buffers alike."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_optim_family_golden as F
import optim_recipe as R

GOLD = F.load()
TOL = 1e-5
DEV = "cuda:0"
NAMES = ("sgd_m09", "sgd_m0", "adam")


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _np(t):
    return t.detach().cpu().numpy()


def _fused(name, ps, lr=R.LR, wd=R.WD):
    from cgat_amd import optim as PO
    if name == "adam":
        return PO.FusedAdam(ps, lr=lr, weight_decay=wd)
    return PO.FusedSGD(ps, lr=lr, weight_decay=wd, momentum=0.9 if name == "sgd_m09" else 0)


def _torch(name, ps, lr=R.LR, wd=R.WD):
    if name == "adam":
        return torch.optim.Adam(ps, lr=lr, weight_decay=wd)
    return torch.optim.SGD(ps, lr=lr, weight_decay=wd, momentum=0.9 if name == "sgd_m09" else 0)


# ---- CPU ----------------------------------------------------------------------------------------------------------

def test_new_entries_refuse_cpu():
    import cgat_amd as P
    for mk in (lambda p: P.FusedSGD([p], lr=0.1), lambda p: P.FusedSGD([p], lr=0.1, momentum=0.9), lambda p: P.FusedAdam([p])):
        p = torch.nn.Parameter(torch.ones(4))
        p.grad = torch.ones(4)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mk(p).step()
    o, s, t = torch.ones(3, 1), torch.zeros(3, 1), torch.zeros(3, 1)
    for kind in F.CRITERIA:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            P.criterion_with_metrics(kind, o, s, t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.L1Loss(o, t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.MSELoss(o, t)
    with pytest.raises(ValueError):
        P.criterion_with_metrics("Huber", o, s, t)


def test_unused_options_are_refused():
    import cgat_amd as P
    p = torch.nn.Parameter(torch.ones(4))
    for kw in (dict(dampening=0.1), dict(nesterov=True, momentum=0.9), dict(maximize=True)):
        with pytest.raises(NotImplementedError):
            P.FusedSGD([p], lr=0.1, **kw)
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(decoupled_weight_decay=True)):
        with pytest.raises(NotImplementedError):
            P.FusedAdam([p], **kw)
    assert not isinstance(P.FusedAdam([p]), P.FusedAdamW)
    adam = P.FusedAdam([p])
    adam.param_groups[0]["decoupled_weight_decay"] = True        # as a state dict of torch.optim.Adam may bring it
    with pytest.raises(NotImplementedError):
        adam.step()
    # ... also when a loaded state dict brings them in
    opt = P.FusedSGD([p], lr=0.1, momentum=0.9)
    opt.load_state_dict(torch.optim.SGD([p], lr=0.1, momentum=0.9, nesterov=True).state_dict())
    with pytest.raises(NotImplementedError):
        opt.step()
    with pytest.raises(NameError, match="SGD, Adam, AdamW"):
        P.DataParallelTrainer(torch.nn.Linear(2, 2), None, optim="RMSprop")


def test_fixture_is_what_torch_computes():
    """Pins that optim_family*.npz is torch's own output: re-running the recipe reproduces it to 2e-6 (the bar of
    test_oracle_optimisers_match_reference), and it holds every case the GPU tests read."""
    again = F.compute()
    assert sorted(again) == sorted(GOLD)
    for k in again:
        assert rel(again[k], GOLD[k]) <= 2e-6, k
    n_params = len(R.SHAPES) + len(F.EXTRA_SHAPES)
    assert [p.numel() for p in F.params()][-2:] == [16384, 16385]
    for name in NAMES:
        for step in (0, R.STEPS - 1):
            assert all(f"{name}.s{step}.p{i}" in GOLD for i in range(n_params))
    assert all(f"sgd_m09.buf.p{i}" in GOLD for i in range(n_params))
    o, _, t = F.loss_inputs()
    assert o.shape == (257, 1) and float(o[5]) == float(((t - F.MEAN) / F.STD)[5])


# ---- optimiser steps ----------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_fused_steps_match_fixture(name):
    ps = [torch.nn.Parameter(t.to(DEV)) for t in F.params()]
    opt = _fused(name, ps)
    for step in range(R.STEPS):
        for i, p in enumerate(ps):
            p.grad = R.grad(i, step, p.shape).to(DEV)
        opt.step()
        if step in (0, R.STEPS - 1):
            for i, p in enumerate(ps):
                assert rel(_np(p), GOLD[f"{name}.s{step}.p{i}"]) <= TOL, (name, step, i)
    if name == "sgd_m09":
        for i, p in enumerate(ps):
            assert rel(_np(opt.state[p]["momentum_buffer"]), GOLD[f"{name}.buf.p{i}"]) <= TOL, (name, "buf", i)
    # a parameter without gradient is untouched, its state included
    ps[1].grad = None
    before = ps[1].detach().clone()
    state_before = {k: v.clone() if torch.is_tensor(v) else v for k, v in opt.state.get(ps[1], {}).items()}
    opt.step()
    assert torch.equal(ps[1].detach(), before)
    for k, v in state_before.items():
        assert torch.equal(opt.state[ps[1]][k], v) if torch.is_tensor(v) else opt.state[ps[1]][k] == v, k


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_fused_steps_match_torch_on_a_model(name):
    """All tensors of CGAtNet(200,64,2): one fused launch per step vs torch's optimiser on the same gradients."""
    import cgat_amd as P
    torch.manual_seed(0)
    net = P.CGAtNet(200, 64, 2, msg_heads=2, neighbor_number=12, update_edges=True).to(DEV)
    ref = copy.deepcopy(net)
    a, b = _fused(name, net.parameters(), 1e-3, 1e-2), _torch(name, ref.parameters(), 1e-3, 1e-2)
    g = torch.Generator().manual_seed(1)
    for step in range(3):
        for p, q in zip(net.parameters(), ref.parameters()):
            gr = torch.randn(p.shape, generator=g).to(DEV)
            p.grad, q.grad = gr.clone(), gr.clone()
        a.step(); b.step()
    for (n, p), q in zip(net.named_parameters(), ref.parameters()):
        assert rel(_np(p), _np(q)) <= TOL, n
        if name == "sgd_m09":
            assert rel(_np(a.state[p]["momentum_buffer"]), _np(b.state[q]["momentum_buffer"])) <= TOL, n


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_torch_state_resumes_in_fused(name):
    """Two torch steps, load_state_dict into the fused optimiser, two more steps against torch (one gradient
    non-contiguous); afterwards the state holds exactly torch's entries."""
    g = torch.Generator().manual_seed(3)
    mk = lambda: [torch.nn.Parameter(torch.randn(s, generator=torch.Generator().manual_seed(7 + i)).to(DEV))
                  for i, s in enumerate([(5, 7), (33,), (128, 4)])]
    ps_t, ps_f = mk(), mk()
    grads = [[torch.randn(p.shape, generator=g).to(DEV) for p in ps_t] for _ in range(4)]
    ref, warm = _torch(name, ps_t, 1e-3, 1e-2), _torch(name, ps_f, 1e-3, 1e-2)
    for step in range(2):
        for opt, ps in ((ref, ps_t), (warm, ps_f)):
            for p, gr in zip(ps, grads[step]):
                p.grad = gr.clone()
            opt.step()
    fused = _fused(name, ps_f, 1e-3, 1e-2)
    fused.load_state_dict(warm.state_dict())
    for step in range(2, 4):
        for p, q, gr in zip(ps_t, ps_f, grads[step]):
            p.grad, q.grad = gr.clone(), gr.t().contiguous().t() if gr.dim() == 2 else gr.clone()
        assert not ps_f[0].grad.is_contiguous()
        ref.step(); fused.step()
    for p, q in zip(ps_t, ps_f):
        assert rel(_np(q), _np(p)) <= TOL
    state = fused.state_dict()["state"]
    if name == "sgd_m0":
        assert state == {}
    else:
        assert len(state) == 3
    for p, st in zip(ps_t, state.values()):
        if name == "adam":
            assert set(st.keys()) == {"step", "exp_avg", "exp_avg_sq"} and int(st["step"]) == 4
        else:
            assert set(st.keys()) == {"momentum_buffer"}
            assert rel(_np(st["momentum_buffer"]), _np(ref.state[p]["momentum_buffer"])) <= TOL


@pytest.mark.gpu
def test_sgd_state_without_buffers_loads():
    """A torch.optim.SGD state taken before its first step (empty), and one that stores `momentum_buffer: None`, load;
    the buffer becomes zeros on first use, which is torch's first step bit for bit in the formula."""
    from cgat_amd import optim as PO
    mk = lambda: [torch.nn.Parameter(t.to(DEV)) for t in R.params()[:3]]
    for with_none in (False, True):
        ps_t, ps_f = mk(), mk()
        ref = torch.optim.SGD(ps_t, lr=R.LR, weight_decay=R.WD, momentum=0.9)
        sd = ref.state_dict()
        assert sd["state"] == {}
        if with_none:
            sd["state"] = {i: {"momentum_buffer": None} for i in range(len(ps_t))}
        fused = PO.FusedSGD(ps_f, lr=1.0, momentum=0.5)
        fused.load_state_dict(sd)                        # brings lr, momentum, weight_decay with it
        for step in range(2):
            for i, (p, q) in enumerate(zip(ps_t, ps_f)):
                p.grad, q.grad = R.grad(i, step, p.shape).to(DEV), R.grad(i, step, p.shape).to(DEV)
            ref.step(); fused.step()
        for p, q in zip(ps_t, ps_f):
            assert rel(_np(q), _np(p)) <= TOL
            assert rel(_np(fused.state[q]["momentum_buffer"]), _np(ref.state[p]["momentum_buffer"])) <= TOL
    assert PO.FusedSGD(mk(), lr=0.1, momentum=0).state_dict()["state"] == {}


@pytest.mark.gpu
def test_adam_group_with_mixed_steps_is_refused():
    from cgat_amd import optim as PO
    ps = [torch.nn.Parameter(torch.ones(4, device=DEV)) for _ in range(2)]
    opt = PO.FusedAdam(ps)
    ps[0].grad = torch.ones(4, device=DEV)
    opt.step()
    ps[1].grad = torch.ones(4, device=DEV)
    with pytest.raises(RuntimeError, match="FusedAdam: parameters of a group must share their step count"):
        opt.step()


# ---- criterion + metrics ------------------------------------------------------------------------------------------

def _fused_criterion(kind, o, s, t, mean, std):
    """(value, go, gs or None, mae, rmse) of criterion_with_metrics, gradients through torch.autograd.grad"""
    import cgat_amd as P
    oo, ss = o.clone().requires_grad_(True), s.clone().requires_grad_(True)
    v, mae, rmse = P.criterion_with_metrics(kind, oo, ss, t, mean, std)
    assert v.dim() == 0 and mae.dim() == 0 and rmse.dim() == 0 and v.requires_grad
    assert not mae.requires_grad and not rmse.requires_grad and mae.is_cuda and rmse.is_cuda
    robust = kind.startswith("Robust")
    g = torch.autograd.grad(v, [oo, ss] if robust else [oo])
    return v, g[0], (g[1] if robust else None), mae, rmse


@pytest.mark.gpu
@pytest.mark.parametrize("kind", F.CRITERIA)
def test_criterion_with_metrics_matches_fixture(kind):
    o, s, t = (x.to(DEV) for x in F.loss_inputs())
    v, go, gs, mae, rmse = _fused_criterion(kind, o, s, t, F.MEAN, F.STD)
    assert rel(_np(v), GOLD[f"{kind}.value"]) <= TOL
    assert go.shape == o.shape and rel(_np(go), GOLD[f"{kind}.go"]) <= TOL
    assert float(go[5]) == 0.0                                                # sign(0) = 0 at the o == t_n row
    if gs is not None:
        assert gs.shape == s.shape and rel(_np(gs), GOLD[f"{kind}.gs"]) <= TOL
    assert rel(_np(mae), GOLD[f"{kind}.mae"]) <= TOL and rel(_np(rmse), GOLD[f"{kind}.rmse"]) <= TOL


@pytest.mark.gpu
def test_criterion_equals_the_packages_losses_and_wrappers():
    import cgat_amd as P
    o, s, t = (x.to(DEV) for x in R.loss_inputs())
    for kind, fn in (("RobustL1", P.RobustL1), ("RobustL2", P.RobustL2)):
        v, go, gs, _, _ = _fused_criterion(kind, o, s, t, 0.0, 1.0)
        oo, ss = o.clone().requires_grad_(True), s.clone().requires_grad_(True)
        w = fn(oo, ss, t)
        wo, ws = torch.autograd.grad(w, [oo, ss])
        assert rel(_np(v), _np(w)) <= TOL and rel(_np(go), _np(wo)) <= TOL and rel(_np(gs), _np(ws)) <= TOL
        # the gradients are the same bits (n = 257): what keeps the trainer's default step unchanged
        assert torch.equal(go, wo) and torch.equal(gs, ws), kind
    for fn, tfn in ((P.L1Loss, torch.nn.L1Loss()), (P.MSELoss, torch.nn.MSELoss())):
        oo, oq = o.clone().requires_grad_(True), o.clone().requires_grad_(True)
        v, w = fn(oo, t), tfn(oq, t)
        assert rel(_np(v), _np(w)) <= TOL
        assert rel(_np(torch.autograd.grad(v, oo)[0]), _np(torch.autograd.grad(w, oq)[0])) <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 4167])
@pytest.mark.parametrize("kind", F.CRITERIA)
def test_criterion_with_metrics_vs_fp64(kind, n):
    """One row, and the 1M-edge batch's crystal count (17 strides of the 256 threads, a 71-row tail), against the torch
    expression evaluated in fp64 on the host."""
    g = torch.Generator().manual_seed(11 + n)
    o, s, t = 2.0 * torch.randn(n, 1, generator=g), 0.7 * torch.randn(n, 1, generator=g), 2.0 * torch.randn(n, 1, generator=g) + 0.5
    od, sd = o.double().requires_grad_(True), s.double().requires_grad_(True)
    robust = kind.startswith("Robust")
    w, wmae, wrmse = F.criterion(kind, od, sd, t.double(), F.MEAN, F.STD)
    wg = torch.autograd.grad(w, [od, sd] if robust else [od])
    v, go, gs, mae, rmse = _fused_criterion(kind, o.to(DEV), s.to(DEV), t.to(DEV), F.MEAN, F.STD)
    print(kind, n, "value", rel(_np(v), _np(w)), "go", rel(_np(go), _np(wg[0])), "mae", rel(_np(mae), _np(wmae)),
          "rmse", rel(_np(rmse), _np(wrmse)))
    assert rel(_np(v), _np(w)) <= TOL and rel(_np(go), _np(wg[0])) <= TOL
    if robust:
        assert rel(_np(gs), _np(wg[1])) <= TOL
    assert rel(_np(mae), _np(wmae)) <= TOL and rel(_np(rmse), _np(wrmse)) <= TOL


@pytest.mark.gpu
def test_criterion_broadcasts_as_the_robust_losses_do():
    """output / log_std [n, 1] against a target [n] broadcast to [n, n], as torch's expression and RobustL1 of this package
    do; the gradients come back reduced to the inputs' shapes."""
    n = 5
    g = torch.Generator().manual_seed(5)
    o, s, t = (torch.randn(sh, generator=g).to(DEV) for sh in ((n, 1), (n, 1), (n,)))
    for kind in F.CRITERIA:
        v, go, gs, mae, rmse = _fused_criterion(kind, o, s, t, F.MEAN, F.STD)
        oo, ss = o.clone().requires_grad_(True), s.clone().requires_grad_(True)
        to, so = torch.broadcast_tensors(oo, t)[0], torch.broadcast_tensors(ss, t)[0]
        w, wmae, wrmse = F.criterion(kind, to, so, t.expand(n, n), F.MEAN, F.STD)
        wg = torch.autograd.grad(w, [oo, ss], allow_unused=True)
        assert go.shape == (n, 1) and rel(_np(v), _np(w)) <= TOL and rel(_np(go), _np(wg[0])) <= TOL
        if gs is not None:
            assert gs.shape == (n, 1) and rel(_np(gs), _np(wg[1])) <= TOL
        assert rel(_np(mae), _np(wmae)) <= TOL and rel(_np(rmse), _np(wrmse)) <= TOL


@pytest.mark.gpu
def test_criterion_with_metrics_never_synchronises_the_host():
    import cgat_amd as P
    o, s, t = (x.to(DEV) for x in F.loss_inputs())
    oo, ss = o.clone().requires_grad_(True), s.clone().requires_grad_(True)
    P.criterion_with_metrics("RobustL1", oo, ss, t, F.MEAN, F.STD)[0].backward()      # warm-up: allocator, autograd
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for kind in F.CRITERIA:
            loss, mae, rmse = P.criterion_with_metrics(kind, oo, ss, t, F.MEAN, F.STD)
            loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(torch.stack([loss.detach(), mae, rmse])).all()


# ---- trainer ------------------------------------------------------------------------------------------------------

def _tiny(seed=0):
    import cgat_amd as P
    from cgat_amd.graph import synthetic_dataset_dict
    data, emb = synthetic_dataset_dict(3, (2, 9), 24, seed=3)
    ds = P.PackedDataset.from_dict(data, emb, max_neighbor_number=12, device=DEV)
    torch.manual_seed(seed)
    net = P.CGAtNet(200, 64, 2, msg_heads=2, neighbor_number=12, update_edges=True).to(DEV)
    return ds, net


def _torch_metrics(net, ds, ids, kind, norm):
    """(loss, mae, rmse) of the torch expressions on `net`'s forward, in its current mode"""
    gb, roost = ds.collate(ids)
    o, s = net(gb, roost).chunk(2, dim=1)
    return F.criterion(kind, o, s, gb.y.view(-1, 1), norm.mean, norm.std)


@pytest.mark.gpu
@pytest.mark.parametrize("optim,std_loss,loss", [("SGD", True, "L1"), ("Adam", True, "L2"), ("AdamW", False, "L2"),
                                                 ("LAMB", False, "L1")])
def test_trainer_steps_with_every_optimiser_and_reports_metrics(optim, std_loss, loss):
    import cgat_amd as P
    ds, net = _tiny()
    norm = P.Normalizer(0.3, 1.7)
    ids = np.arange(3)
    kind = ("" if std_loss else "Robust") + loss
    want = [float(x.detach()) for x in _torch_metrics(copy.deepcopy(net), ds, ids, kind, norm)]
    tr = P.DataParallelTrainer(net, ds, lr=1e-3, weight_decay=1e-2, loss=loss, normalizer=norm, optim=optim,
                               std_loss=std_loss)
    assert type(tr.optimizer).__name__ == {"SGD": "FusedSGD", "Adam": "FusedAdam", "AdamW": "FusedAdamW", "LAMB": "FusedLamb"}[optim]
    if optim == "SGD":
        assert tr.optimizer.param_groups[0]["momentum"] == 0.9
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    out, edges = tr.step(ids)
    changed = [n for n, p in net.named_parameters() if not torch.equal(p.detach(), before[n])]
    assert changed and all(dict(net.named_parameters())[n].grad is not None for n in changed)
    m = tr.last_metrics
    assert set(m) == {"loss", "mae", "rmse"} and all(v.is_cuda and v.dim() == 0 and not v.requires_grad for v in m.values())
    assert torch.equal(m["loss"], out)
    got = [float(m[k]) for k in ("loss", "mae", "rmse")]
    print(optim, kind, got, want)
    for a, b in zip(got, want):
        assert abs(a - b) <= TOL * abs(b), (got, want)


@pytest.mark.gpu
def test_trainer_only_residual_trains_the_output_network_alone():
    import cgat_amd as P
    ds, net = _tiny()
    tr = P.DataParallelTrainer(net, ds, lr=1e-3, weight_decay=1e-2, only_residual=True)
    outs = {id(p) for p in net.get_output_parameters()}
    assert {id(p) for g in tr.optimizer.param_groups for p in g["params"]} == outs
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    tr.step(np.arange(3))
    named = dict(net.named_parameters())
    changed = {n for n, p in named.items() if not torch.equal(p.detach(), before[n])}
    # AdamW leaves a tensor in place only where both it and its gradient are zero
    movable = {n for n, p in named.items() if id(p) in outs and (float(before[n].abs().max()) > 0 or float(p.grad.abs().max()) > 0)}
    assert changed == movable and len(changed) >= 2
    # gradients are still formed for the rest of the network, as in the reference
    assert any(p.grad is not None and float(p.grad.abs().max()) > 0 for n, p in named.items() if id(p) not in outs)


@pytest.mark.gpu
@pytest.mark.parametrize("training", [True, False])
def test_trainer_validate_touches_nothing(training):
    import cgat_amd as P
    ds, net = _tiny()
    norm = P.Normalizer(0.3, 1.7)
    tr = P.DataParallelTrainer(net, ds, lr=1e-3, weight_decay=1e-2, normalizer=norm, optim="SGD")
    ids = np.arange(3)
    tr.step(ids)
    net.train(training)
    params = [p.detach().clone() for p in net.parameters()]
    grads = [None if p.grad is None else p.grad.clone() for p in net.parameters()]
    state = copy.deepcopy(tr.optimizer.state_dict())
    metrics = dict(tr.last_metrics)
    got = tr.validate(ids)
    assert net.training is training and all(m.training is training for m in net.modules())
    for p, q, g in zip(net.parameters(), params, grads):
        assert torch.equal(p.detach(), q)
        assert (p.grad is None and g is None) or torch.equal(p.grad, g)
    after = tr.optimizer.state_dict()
    assert after["param_groups"] == state["param_groups"] and after["state"].keys() == state["state"].keys()
    for k, st in after["state"].items():
        assert st.keys() == state["state"][k].keys() and all(torch.equal(st[j], state["state"][k][j]) for j in st)
    assert all(tr.last_metrics[k] is metrics[k] for k in metrics)
    ref = copy.deepcopy(net).eval()
    with torch.no_grad():
        want = _torch_metrics(ref, ds, ids, "RobustL1", norm)
    assert all(not x.requires_grad and x.is_cuda and x.dim() == 0 for x in got)
    for a, b in zip(got, want):
        assert abs(float(a) - float(b)) <= TOL * abs(float(b)), ([float(x) for x in got], [float(x) for x in want])


@pytest.mark.gpu
def test_default_trainer_is_the_adamw_robust_l1_step_bit_for_bit():
    """The defaults keep the step this trainer took before it had choices: FusedAdamW on RobustL1 of the normalised
    target, composed here from the package's own pieces; identical parameters after two steps."""
    import cgat_amd as P
    ds, net = _tiny()
    ref = copy.deepcopy(net)
    tr = P.DataParallelTrainer(net, ds, lr=1e-3, weight_decay=1e-2)
    opt = P.FusedAdamW([p for p in ref.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-2)
    norm = P.Normalizer()
    for ids in (np.arange(3), np.array([2, 0])):
        tr.step(ids)
        for p in ref.parameters():
            p.grad = None
        gb, roost = ds.collate(ids)
        o, s = ref(gb, roost).chunk(2, dim=1)
        P.RobustL1(o, s, norm.norm(gb.y.view(-1, 1))).backward()
        opt.step()
    for (n, p), q in zip(net.named_parameters(), ref.parameters()):
        assert torch.equal(p.detach(), q.detach()), n
