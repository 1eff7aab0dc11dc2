"""optim.SparseGaussianAdam (csrc/adam.hip adam_step_rows_kernel, gsr_adam_step_rows) on the GPU.

The oracle is torch.optim.Adam (default foreach) on clones, stepped densely with the same gradients; the expected
result is where(row visible, dense result, state before) for the parameter and both moments, compared as int32 so
that NaN payloads count.  Then: poisoned invisible rows, unaligned tensors, the equivalences with the dense step,
skipped parameters and a changed P, optimizer-state surgery and state_dict interchange, the trainer with
optimizer_type="sparse_adam" against a restatement from torch ops, and checkpoint / resume."""
import copy
import os
import sys
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "examples"))

from mvs_gaussian_splatting_amd import optim  # noqa: E402
from mvs_gaussian_splatting_amd.densify import densify_and_prune, FORK_ATTR, FORK_FLAG, GROUP_ATTR  # noqa: E402
from mvs_gaussian_splatting_amd.layout import reorder_gaussians_  # noqa: E402

# arguments/__init__.py:82-107, the reference's defaults
OPT = types.SimpleNamespace(percent_dense=0.01, position_lr_init=0.00016, position_lr_final=0.0000016,
                            position_lr_delay_mult=0.01, position_lr_max_steps=30_000, feature_lr=0.0025,
                            opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001, growdirs_lr=0.005,
                            growdistance_lr=0.001, splitdistance_lr=0.005, splitscale_lr=0.005,
                            opacity_reset_interval=3000)
WIDTH = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,),
         "dirs_prob": (128,), "conti_dirs": (3,), "grow_dist": (1,), "split_distance": (3,), "split_scale": (1,)}
CHUNK = 4096                                                     # elements a block of the kernel takes
NAN_PAYLOAD = 0x7FC12345                                         # a quiet NaN with a payload a float op would lose


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _row_floats(k):
    n = 1
    for w in WIDTH[k]:
        n *= w
    return n


def _model(P, dev, fork=(), seed=0):
    """A duck-typed GaussianModel: the six plain tensors plus the fork's learned tensors of `fork`, as leaves."""
    g = torch.Generator().manual_seed(seed)
    m = types.SimpleNamespace(spatial_lr_scale=2.5, num_dirs=128, modelcg=types.SimpleNamespace())
    for k, a in GROUP_ATTR.items():
        t = torch.randn((P,) + WIDTH[k], generator=g)
        if k == "scaling":
            t = t * 0.5 + torch.log(torch.tensor(0.05))
        setattr(m, a, torch.nn.Parameter(t.to(dev)))
    for k, a in FORK_ATTR.items():
        on = k in fork
        setattr(m, FORK_FLAG[k], on)
        if on:
            setattr(m, a, torch.nn.Parameter(torch.randn((P,) + WIDTH[k], generator=g).to(dev)))
    if "dirs_prob" in fork:
        d = torch.randn(128, 3, generator=g)
        m.dirs = (d / d.norm(dim=1, keepdim=True)).to(dev)
    for f in ("symmetric_split", "split_notreinit", "prob_notreinit"):
        setattr(m.modelcg, f, False)
    m.max_radii2D = torch.zeros(P, device=dev)
    return m


def _clone_model(m):
    c = copy.copy(m)
    for a in list(GROUP_ATTR.values()) + list(FORK_ATTR.values()):
        t = getattr(m, a, None)
        if isinstance(t, torch.Tensor):
            setattr(c, a, torch.nn.Parameter(t.detach().clone()))
    return c


def _pair(P, dev, fork=(), seed=0, cls=None):
    """(oracle model with torch.optim.Adam, model under test with SparseGaussianAdam), equal parameters."""
    a = _model(P, dev, fork, seed)
    b = _clone_model(a)
    optim.training_setup(a, OPT, torch.optim.Adam)
    optim.training_setup(b, OPT, cls or optim.SparseGaussianAdam)
    return a, b


def _grads(model, it, skip=()):
    """Fresh gradients for every group, the same for both runs: normal values with some zero rows and some tiny and
    huge magnitudes; groups in `skip` get grad = None."""
    g = torch.Generator(device=model._xyz.device).manual_seed(1000 + it)
    for grp in model.optimizer.param_groups:
        p = grp["params"][0]
        if grp["name"] in skip:
            p.grad = None
            continue
        x = torch.randn(p.shape, generator=g, device=p.device)
        flat = x.view(-1)
        n = flat.numel()
        flat[0:n:11] = 0.0
        flat[1:n:13] *= 1e-30
        flat[2:n:17] *= 1e15
        flat[3:n:19] *= 1e-7
        p.grad = x


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _oracle_step(model, rows, dense=()):
    """One dense torch.optim.Adam step, then the rows outside the bool mask `rows` put back as they were: parameter
    and both moments (zeros where the state is new), moved as int32.  Groups named in `dense` keep the dense result."""
    opt = model.optimizer
    before = {}
    for grp in opt.param_groups:
        p = grp["params"][0]
        if p.grad is None:
            continue
        st = opt.state.get(p, {})
        before[p] = [p.detach().clone()] + [st[k].clone() if k in st else torch.zeros_like(p)
                                            for k in ("exp_avg", "exp_avg_sq")]
    opt.step()
    for grp in opt.param_groups:
        p = grp["params"][0]
        if p not in before or grp["name"] in dense:
            continue
        keep = rows.view((-1,) + (1,) * (p.dim() - 1))
        st = opt.state[p]
        for now, old in zip((p.data, st["exp_avg"], st["exp_avg_sq"]), before[p]):
            now.view(torch.int32).copy_(torch.where(keep, now.view(torch.int32), old.view(torch.int32)))


def _assert_same(ma, mb, what):
    oa, ob = ma.optimizer, mb.optimizer
    assert [g["name"] for g in oa.param_groups] == [g["name"] for g in ob.param_groups]
    for ga, gb in zip(oa.param_groups, ob.param_groups):
        pa, pb = ga["params"][0], gb["params"][0]
        assert torch.equal(_bits(pa), _bits(pb)), f"{what}: param {ga['name']} differs"
        sa, sb = oa.state.get(pa, {}), ob.state.get(pb, {})
        assert set(sa) == set(sb), f"{what}: state keys of {ga['name']}"
        for key in ("exp_avg", "exp_avg_sq"):
            if key in sa:
                assert torch.equal(_bits(sa[key]), _bits(sb[key])), f"{what}: {key} of {ga['name']} differs"
        if "step" in sa:
            assert sa["step"].dtype == sb["step"].dtype == torch.float32 and not sb["step"].is_cuda
            assert float(sa["step"]) == float(sb["step"]), f"{what}: step of {ga['name']}"


def _boundary_rows(P, names):
    """The row that holds the first element of every 4096-element chunk, for every row width in use."""
    rows = set()
    for k in names:
        w = _row_floats(k)
        rows.update((c * CHUNK) // w for c in range(1, (P * w + CHUNK - 1) // CHUNK))
    return sorted(r for r in rows if r < P)


def _mask(name, P, names, seed=0):
    m = torch.zeros(P, dtype=torch.bool)
    if name == "none":
        pass
    elif name == "all":
        m[:] = True
    elif name == "first":
        m[0] = True
    elif name == "last":
        m[-1] = True
    elif name == "alternating":
        m[::2] = True
    elif name == "seeded35":
        m = torch.rand(P, generator=torch.Generator().manual_seed(seed)) < 0.35
    elif name == "block":
        m[P // 3:P // 3 + max(P // 4, 1)] = True
    elif name == "all_but_boundaries":
        m[:] = True
        m[_boundary_rows(P, names)] = False
    else:
        raise KeyError(name)
    return m


def _visibility(rows, kind, dev, seed=0):
    """The bool mask as the tensor a caller would pass: bool, uint8 with any non-zero value, or int32 'radii' with
    zeros and negatives for the invisible."""
    g = torch.Generator().manual_seed(seed)
    P = rows.numel()
    if kind == "bool":
        v = rows.clone()
    elif kind == "uint8":
        v = torch.where(rows, torch.randint(1, 256, (P,), generator=g), torch.zeros(P, dtype=torch.int64)).to(torch.uint8)
    else:
        hidden = torch.tensor([0, -1, -7, -2**31])[torch.randint(0, 4, (P,), generator=g)]
        v = torch.where(rows, torch.randint(1, 2000, (P,), generator=g), hidden).to(torch.int32)
        assert torch.equal(v > 0, rows)
    return v.to(dev)


def _step_both(a, b, it, rows, kind, skip=(), dense=()):
    dev = b._xyz.device
    for m in (a, b):
        _grads(m, it, skip)
    _oracle_step(a, rows.to(dev), dense)
    b.optimizer.step(_visibility(rows, kind, dev, seed=it), dense=dense)
    for m in (a, b):
        m.optimizer.zero_grad(set_to_none=True)


SEQUENCES = {"edges": ("none", "all", "first"), "scattered": ("last", "alternating", "seeded35"),
             "runs": ("block", "all_but_boundaries", "seeded35")}


# ---- 1. the defining property ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", [("bool", "uint8", "bool"), ("int32",) * 3], ids=["bytes", "int32"])
@pytest.mark.parametrize("seq", sorted(SEQUENCES))
@pytest.mark.parametrize("P", [1, 7, 4097, 100_003])
def test_visible_rows_get_the_dense_step_and_the_others_keep_their_bits(dev, P, seq, kinds):
    fork = tuple(FORK_ATTR)
    a, b = _pair(P, dev, fork, seed=P % 97)
    names = [g["name"] for g in b.optimizer.param_groups]
    assert len(names) == 11 and sorted(_row_floats(k) for k in names) == [1, 1, 1, 3, 3, 3, 3, 3, 4, 45, 128]
    for it, (mask, kind) in enumerate(zip(SEQUENCES[seq], kinds)):
        optim.update_learning_rate(a, 500 * it)
        optim.update_learning_rate(b, 500 * it)
        rows = _mask(mask, P, names, seed=it)
        _step_both(a, b, it, rows, kind)
        _assert_same(a, b, f"P={P} step {it} ({mask}, {kind})")
        for g in b.optimizer.param_groups:
            assert float(b.optimizer.state[g["params"][0]]["step"]) == it + 1   # counted on every call, seen or not


def test_a_45_float_row_across_a_chunk_boundary_with_one_side_visible(dev):
    """At P = 4097 the row of f_rest that holds element 4096 starts in one block's chunk and ends in the next one's,
    and the 16-byte piece before the boundary is shared with the row in front of it."""
    P, w = 4097, _row_floats("f_rest")
    r = CHUNK // w                                               # the row element 4096 lies in
    assert r * w < CHUNK < (r + 1) * w and (r * w) % 4 != 0      # it straddles, and so does a 16-byte piece
    for it, visible in enumerate(([r], [r - 1, r + 1], [r - 1], [r + 1])):
        a, b = _pair(P, dev, seed=3)
        rows = torch.zeros(P, dtype=torch.bool)
        rows[visible] = True
        start = b._features_rest.detach().clone()
        _step_both(a, b, 0, rows, "int32" if it % 2 else "bool")
        _assert_same(a, b, f"rows {visible} visible")
        moved = (_bits(b._features_rest) != _bits(start)).view(P, -1).any(dim=1).cpu()
        assert moved[visible].all() and int(moved.sum()) == len(visible)


def test_rows_longer_than_a_chunk(dev):
    """A row of 5000 floats meets a chunk in at most two rows: the kernel's other way to find a row."""
    g = torch.Generator().manual_seed(1)
    for it, P in enumerate((1, 3, 6)):
        base = torch.randn(P, 5000, generator=g).to(dev)
        pa, pb = torch.nn.Parameter(base.clone()), torch.nn.Parameter(base.clone())
        a = types.SimpleNamespace(optimizer=torch.optim.Adam([{"params": [pa], "name": "wide"}], lr=1e-2, eps=1e-15))
        b = types.SimpleNamespace(optimizer=optim.SparseGaussianAdam([{"params": [pb], "name": "wide"}], lr=1e-2, eps=1e-15),
                                  _xyz=pb)
        a._xyz = pa
        for step, rows in enumerate((torch.arange(P) % 2 == 0, torch.arange(P) % 2 == 1, torch.ones(P, dtype=torch.bool))):
            _step_both(a, b, step, rows, ("bool", "int32", "uint8")[step])
            _assert_same(a, b, f"P={P} step {step}")


# ---- 2. poison ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bool", "int32"])
def test_poisoned_invisible_rows_leak_nothing_and_keep_their_payloads(dev, kind):
    P = 4097
    a, b = _pair(P, dev, ("dirs_prob", "grow_dist"), seed=11)
    names = [g["name"] for g in b.optimizer.param_groups]
    masks = [_mask(m, P, names, seed=40 + i) for i, m in enumerate(("seeded35", "alternating", "block"))]
    for m in masks:
        m[_boundary_rows(P, names)] = False                      # poison next to every chunk boundary too
    never = (~(masks[0] | masks[1] | masks[2])).nonzero().flatten()[0::2]   # rows that hold NaNs with a payload
    assert never.numel() > 100
    for it, rows in enumerate(masks):
        hidden = (~rows).nonzero().flatten()
        for m in (a, b):
            _grads(m, it)
            for grp in m.optimizer.param_groups:
                p = grp["params"][0]
                g2 = p.grad.view(P, -1)
                g2[hidden[0::3]] = float("nan")
                g2[hidden[1::3]] = float("inf")
                g2[hidden[2::3]] = 1e38
                targets = [p.data] + [m.optimizer.state[p][k] for k in ("exp_avg", "exp_avg_sq") if p in m.optimizer.state]
                for t in targets:                                # the moments too, once they exist
                    t.view(torch.int32).view(P, -1)[never] = NAN_PAYLOAD
        _oracle_step(a, rows.to(dev))
        b.optimizer.step(_visibility(rows, kind, dev, seed=it))
        _assert_same(a, b, f"poison step {it}")
        for grp in b.optimizer.param_groups:
            p = grp["params"][0]
            tensors = (p.data, b.optimizer.state[p]["exp_avg"], b.optimizer.state[p]["exp_avg_sq"])
            for t in tensors:
                assert torch.isfinite(t.view(P, -1)[rows.to(dev)]).all(), f"{grp['name']}: a visible row caught the poison"
            for t in tensors[:1] if it == 0 else tensors:
                assert (_bits(t).view(P, -1)[never.to(dev)] == NAN_PAYLOAD).all(), f"{grp['name']}: a payload was lost"


# ---- 3. unaligned ---------------------------------------------------------------------------------------------------
def test_tensors_at_a_4_byte_offset(dev):
    P = 4097
    g = torch.Generator().manual_seed(5)
    pa, pb = [], []
    for k in ("xyz", "f_rest", "opacity", "rotation", "dirs_prob"):
        w = _row_floats(k)
        base = torch.randn(P * w + 9, generator=g).to(dev)
        pa.append(torch.nn.Parameter(base[1:1 + P * w].clone().view(P, w)))
        pb.append(torch.nn.Parameter(base.clone()[1:1 + P * w].view(P, w)))       # a view 4 bytes into its storage
        assert pb[-1].data_ptr() % 16 == 4 and pb[-1].is_contiguous()
    names = ("xyz", "f_rest", "opacity", "rotation", "dirs_prob")
    a = types.SimpleNamespace(_xyz=pa[0], optimizer=torch.optim.Adam(
        [{"params": [p], "name": n} for p, n in zip(pa, names)], lr=1e-2, eps=1e-15))
    b = types.SimpleNamespace(_xyz=pb[0], optimizer=optim.SparseGaussianAdam(
        [{"params": [p], "name": n} for p, n in zip(pb, names)], lr=1e-2, eps=1e-15))
    for it, (mask, kind) in enumerate((("seeded35", "bool"), ("all_but_boundaries", "int32"), ("alternating", "uint8"))):
        rows = _mask(mask, P, names, seed=it)
        _step_both(a, b, it, rows, kind)
        if it == 0:                                              # the moments too, from the second step on
            for p in pb:
                for key in ("exp_avg", "exp_avg_sq"):
                    old = b.optimizer.state[p][key]
                    buf = torch.zeros(old.numel() + 9, device=dev)
                    buf[1:1 + old.numel()] = old.view(-1)
                    b.optimizer.state[p][key] = buf[1:1 + old.numel()].view(old.shape)
        _assert_same(a, b, f"unaligned step {it}")


# ---- 4. equivalences ------------------------------------------------------------------------------------------------
def test_no_visibility_and_all_visible_are_the_dense_step(dev):
    P = 5003
    fork = tuple(FORK_ATTR)
    ref = _model(P, dev, fork, seed=2)
    none, ones = _clone_model(ref), _clone_model(ref)
    optim.training_setup(ref, OPT, optim.Adam)
    optim.training_setup(none, OPT, optim.SparseGaussianAdam)
    optim.training_setup(ones, OPT, optim.SparseGaussianAdam)
    for it in range(4):
        for m in (ref, none, ones):
            _grads(m, it, skip=("scaling",) if it == 2 else ())
        ref.optimizer.step()
        none.optimizer.step()
        ones.optimizer.step(_visibility(torch.ones(P, dtype=torch.bool), ("bool", "int32")[it % 2], dev))
        _assert_same(ref, none, f"visibility=None, step {it}")
        _assert_same(ref, ones, f"all visible, step {it}")


def test_dense_groups_take_the_dense_update_in_the_same_step(dev):
    P = 4097
    a, b = _pair(P, dev, ("grow_dist",), seed=8)
    names = [g["name"] for g in b.optimizer.param_groups]
    for it, dense in enumerate((("opacity",), ("opacity", "grow_dist"), ())):
        rows = _mask("seeded35", P, names, seed=it)
        before = b._opacity.detach().clone()
        _step_both(a, b, it, rows, "bool", dense=dense)
        _assert_same(a, b, f"dense={dense}")
        if "opacity" in dense:
            assert (b._opacity.detach() != before)[~rows.to(dev)].any()         # invisible rows moved there


# ---- 5. skipped parameters, changed P -------------------------------------------------------------------------------
def test_skipped_parameters_and_a_visibility_of_the_wrong_length(dev):
    P = 1000
    a, b = _pair(P, dev, ("dirs_prob",), seed=4)
    names = [g["name"] for g in b.optimizer.param_groups]
    rows = _mask("seeded35", P, names)
    _step_both(a, b, 0, rows, "bool")
    _step_both(a, b, 1, rows, "int32", skip=("f_rest", "dirs_prob"))
    _assert_same(a, b, "with skipped groups")
    steps = {g["name"]: float(b.optimizer.state[g["params"][0]]["step"]) for g in b.optimizer.param_groups}
    assert steps["xyz"] == 2 and steps["f_rest"] == 1 and steps["dirs_prob"] == 1
    # P changed under the caller (a densification): a visibility of the old length is refused before anything moves
    snapshot = copy.deepcopy(b.optimizer.state_dict()["state"])
    params = [g["params"][0].detach().clone() for g in b.optimizer.param_groups]
    _grads(b, 2)
    for bad in (torch.ones(P - 1, dtype=torch.bool, device=dev), torch.ones(P + 5, dtype=torch.int32, device=dev)):
        with pytest.raises(ValueError):
            b.optimizer.step(bad)
    with pytest.raises(ValueError):
        b.optimizer.step(torch.ones(P, dtype=torch.bool))       # on the CPU
    now = b.optimizer.state_dict()["state"]
    for k in snapshot:
        assert float(now[k]["step"]) == float(snapshot[k]["step"])
        assert torch.equal(now[k]["exp_avg"], snapshot[k]["exp_avg"])
        assert torch.equal(now[k]["exp_avg_sq"], snapshot[k]["exp_avg_sq"])
    for g, p in zip(b.optimizer.param_groups, params):
        assert torch.equal(g["params"][0], p)
    # with no gradient anywhere the length is not looked at: the iteration after a densification
    b.optimizer.zero_grad(set_to_none=True)
    b.optimizer.step(torch.ones(P - 1, dtype=torch.bool, device=dev))
    assert all(float(now[k]["step"]) == float(snapshot[k]["step"]) for k in snapshot)
    fresh = optim.SparseGaussianAdam([torch.nn.Parameter(torch.zeros(3, 3, device=dev))], lr=0.1)
    fresh.step(torch.ones(7, dtype=torch.bool, device=dev))
    assert len(fresh.state) == 0


# ---- 6. surgery and interchange -------------------------------------------------------------------------------------
@pytest.mark.parametrize("fork", [(), ("dirs_prob", "grow_dist", "split_distance", "split_scale")])
def test_state_surgery_then_continue(dev, fork):
    a, b = _pair(3000, dev, fork, seed=5)
    it = 0
    for phase in ("densify", "reorder", "end"):
        for _ in range(2):
            P = b._xyz.shape[0]
            names = [g["name"] for g in b.optimizer.param_groups]
            _step_both(a, b, it, _mask(("seeded35", "block", "alternating")[it % 3], P, names, seed=it),
                       ("bool", "int32")[it % 2])
            it += 1
        for m in (a, b):
            g = torch.Generator().manual_seed(77 + it)
            P = m._xyz.shape[0]
            m.denom = torch.randint(0, 4, (P, 1), generator=g).float().to(dev)
            m.xyz_gradient_accum = (torch.rand(P, 1, generator=g) * 0.0006).to(dev) * m.denom
            if phase == "densify":
                torch.manual_seed(11 + it)                     # the split's (and re-init's) draws, the same for both
                densify_and_prune(m, 0.0002, 0.005, 5.0, 20, opt=OPT, iteration=3100)
            elif phase == "reorder":
                reorder_gaussians_(m)
        _assert_same(a, b, f"after {phase}")
    assert a._xyz.shape[0] != 3000 and isinstance(b.optimizer, optim.SparseGaussianAdam)


def test_state_dict_interchange(dev):
    P = 20000
    a, b = _pair(P, dev, ("dirs_prob",), seed=9)
    names = [g["name"] for g in b.optimizer.param_groups]
    masks = [_mask("seeded35", P, names, seed=s) for s in range(6)]
    for it in range(2):
        _step_both(a, b, it, masks[it], "bool")
    # sparse -> torch.optim.Adam: the oracle's own recipe runs on the test's model from here
    sd = b.optimizer.state_dict()
    b.optimizer = torch.optim.Adam(optim.param_groups(b, OPT), lr=0.0, eps=1e-15)
    b.optimizer.load_state_dict(sd)
    for it in range(2, 4):
        for m in (a, b):
            _grads(m, it)
            _oracle_step(m, masks[it].to(dev))
            m.optimizer.zero_grad(set_to_none=True)
    _assert_same(a, b, "sparse -> torch")
    sd = b.optimizer.state_dict()
    b.optimizer = optim.SparseGaussianAdam(optim.param_groups(b, OPT), lr=0.0, eps=1e-15)
    b.optimizer.load_state_dict(sd)
    for it in range(4, 6):
        _step_both(a, b, it, masks[it], "int32")
    _assert_same(a, b, "torch -> sparse")


# ---- 7. the trainer -------------------------------------------------------------------------------------------------
class WhereAdam(torch.optim.Adam):
    """SparseGaussianAdam restated from torch ops for the trainer: torch's dense step, then where() with the frame's
    mask puts the other rows back.  `masks` records what the trainer passed."""
    masks = None

    @torch.no_grad()
    def step(self, visibility=None, dense=(), closure=None):
        if visibility is None:
            return super().step(closure)
        if self.masks is not None:
            self.masks.append((visibility.clone(), tuple(dense)))
        _oracle_step(types.SimpleNamespace(optimizer=_Plain(self)), visibility > 0, dense)
        return None


class _Plain:
    """The dense step of the torch.optim.Adam underneath a WhereAdam."""
    def __init__(self, opt):
        self.param_groups, self.state = opt.param_groups, opt.state
        self.step = lambda: torch.optim.Adam.step(opt)


def _example():
    import train as example
    return example


def _trainer_opt(ex, kind, **over):
    """40 iterations, 991..1030: the SH step of iteration 1000, densifications at 1000, 1010 and 1020, the opacity reset
    at 1020."""
    from mvs_gaussian_splatting_amd.trainer import OptimizationParams
    kw = dict(iterations=2000, position_lr_max_steps=2000, densify_from_iter=990, densification_interval=10,
              opacity_reset_interval=340, densify_until_iter=1025, densify_grad_threshold=0.0002, optimizer_type=kind)
    kw.update(over)
    return OptimizationParams(**kw)


def _params(model):
    out = {g["name"]: g["params"][0].detach().clone() for g in model.optimizer.param_groups}
    for g in model.optimizer.param_groups:
        st = model.optimizer.state.get(g["params"][0], {})
        for k in ("exp_avg", "exp_avg_sq"):
            if k in st:
                out[g["name"] + "/" + k] = st[k].clone()
    return out


def _same_params(x, y):
    return x.keys() == y.keys() and all(x[k].shape == y[k].shape and torch.equal(_bits(x[k]), _bits(y[k])) for k in x)


def test_trainer_sparse_adam_is_repeatable_differs_from_default_and_equals_its_restatement(dev):
    ex = _example()
    problem = ex.make_problem(dev)
    dataset = types.SimpleNamespace(white_background=False)
    runs, events = {}, {}
    for name, kind, cls in (("sparse", "sparse_adam", None), ("again", "sparse_adam", None), ("default", "default", None),
                            ("where", "sparse_adam", WhereAdam)):
        opt = _trainer_opt(ex, kind)
        model = ex.make_model(problem, opt, dataset, optimizer_cls=cls)
        assert type(model.optimizer) is {"sparse": optim.SparseGaussianAdam, "again": optim.SparseGaussianAdam,
                                         "default": optim.Adam, "where": WhereAdam}[name]
        seen = []
        ex.train(model, problem, opt, 990, 1030, dataset=dataset,
                 on_iteration=lambda it, m: seen.append((m._xyz.shape[0], m.active_sh_degree)))
        runs[name], events[name] = _params(model), seen
    sizes = [s for s, _ in events["sparse"]]
    assert len(set(sizes)) > 1, "the window must hold a densification that changes the model"
    assert [d for _, d in events["sparse"]][0] == 0 and events["sparse"][-1][1] == 1, "the window must hold an SH step"
    assert _same_params(runs["sparse"], runs["again"]), "two sparse_adam runs differ"
    assert not _same_params(runs["sparse"], runs["default"]), "sparse_adam gave the dense run: nothing was culled"
    assert events["where"] == events["sparse"]
    assert _same_params(runs["sparse"], runs["where"]), "sparse_adam differs from torch Adam + where(visibility_filter)"


GROW = types.SimpleNamespace(white_background=False, grow_dir=True, num_dirs=32, continous_dir=False,
                             grow_distance=True, learn_split_distance=True, learn_split_scale=True,
                             symmetric_split=False, split_notreinit=False, prob_notreinit=False)


def test_trainer_passes_visibility_or_selected_on_a_grown_frame(dev, monkeypatch):
    """On a grown / learned-split frame a selected source row gets the folded gradient of its virtual copy even when it
    is off screen itself: the mask is visibility_filter | selected_pts_mask, and such a row moves."""
    from mvs_gaussian_splatting_amd import trainer
    ex = _example()
    problem = ex.make_problem(dev, P=1500, W=128, H=80, n_views=4)
    opt = ex.small_opt(40, densify_grad_threshold=0.0002, densify_from_iter=10, densification_interval=20,
                       opacity_reset_interval=30, densify_until_iter=31, optimizer_type="sparse_adam")
    frames = []
    real_render = trainer.render

    def spy(*args, **kw):
        pkg = real_render(*args, **kw)
        frames.append((pkg["visibility_filter"].clone(),
                       None if pkg["selected_pts_mask"] is None else pkg["selected_pts_mask"].clone()))
        return pkg
    monkeypatch.setattr(trainer, "render", spy)
    model = ex.make_model(problem, opt, GROW)
    passed, moved_off_screen = [], 0
    real_step = optim.SparseGaussianAdam.step

    def step_spy(self, visibility=None, dense=(), closure=None):
        passed.append(visibility.clone())
        return real_step(self, visibility, dense, closure)
    monkeypatch.setattr(optim.SparseGaussianAdam, "step", step_spy)
    for it in range(1, 40):                                      # iteration 40 = opt.iterations does not step
        before = {g["name"]: g["params"][0].detach().clone() for g in model.optimizer.param_groups}
        ex.train(model, problem, opt, it - 1, it, dataset=GROW)
        assert len(passed) == len(frames) == it
        vis, sel = frames[-1]
        want = vis if sel is None else vis | sel
        assert passed[-1].dtype == torch.bool and passed[-1].shape == want.shape, (it, passed[-1].shape, want.shape)
        assert torch.equal(passed[-1], want), (it, int((passed[-1] != want).sum()), sel is None)
        todo = trainer.schedule(opt, it, False)
        if sel is None or todo["densify"] or todo["reset"]:
            continue
        off = sel & ~vis
        if off.any():
            changed = torch.zeros_like(off)
            for g in model.optimizer.param_groups:
                changed |= (_bits(g["params"][0]) != _bits(before[g["name"]])).view(off.numel(), -1).any(dim=1)
            assert changed[off].any(), "a selected, off-screen source row did not move"
            assert not changed[~want].any(), "a row outside visibility | selected moved"
            moved_off_screen += int(off.sum())
    assert any(s is not None for _, s in frames), "no grown frame in the window"
    assert moved_off_screen > 0, "no grown frame had a selected source off screen"


def test_trainer_steps_opacity_densely_under_the_sparsity_term(dev, monkeypatch):
    """opacitysparse > 0: the term's gradient lands on low-opacity rows whether the frame saw them or not, so the
    opacity group takes the dense step -- an off-screen low-opacity row's opacity moves, its xyz does not."""
    from mvs_gaussian_splatting_amd import trainer
    ex = _example()
    problem = ex.make_problem(dev, P=1500, W=128, H=80, n_views=4)
    opt = ex.small_opt(6, opacitysparse=0.05, optimizer_type="sparse_adam", densify_from_iter=100, densify_until_iter=200,
                       opacity_reset_interval=1000)
    model = ex.make_model(problem, opt)
    with torch.no_grad():
        model._opacity[::3] = -6.0                               # sigmoid(-6) < 0.005: rows the sparsity term acts on
        model._xyz[0:60:3] = torch.tensor([50.0, 0.0, 4.0], device=dev)   # some of them far outside every frustum
    frames = []
    real_render = trainer.render

    def spy(*args, **kw):
        pkg = real_render(*args, **kw)
        frames.append(pkg["visibility_filter"].clone())
        return pkg
    monkeypatch.setattr(trainer, "render", spy)
    hits = 0
    for it in range(1, 5):
        xyz, opacity = model._xyz.detach().clone(), model._opacity.detach().clone()
        ex.train(model, problem, opt, it - 1, it)
        low_off = ~frames[-1] & (torch.sigmoid(opacity[:, 0]) < 0.005)
        assert low_off.any(), "the frame must leave low-opacity rows off screen"
        assert (model._opacity.detach() != opacity)[low_off].any(), "no off-screen low-opacity row's opacity moved"
        assert torch.equal(model._xyz.detach()[~frames[-1]], xyz[~frames[-1]]), "an off-screen row's xyz moved"
        assert not torch.equal(model._xyz.detach()[frames[-1]], xyz[frames[-1]])
        hits += int(low_off.sum())
    assert hits > 0


# ---- 8. checkpoint --------------------------------------------------------------------------------------------------
def test_checkpoint_and_resume_is_bit_identical_under_sparse_adam(dev, tmp_path):
    from mvs_gaussian_splatting_amd.trainer import load_checkpoint, save_checkpoint
    ex = _example()
    K = 20
    dataset = types.SimpleNamespace(white_background=False)
    opt = ex.small_opt(2 * K, opacitysparse=0.05, densify_grad_threshold=0.0002, densify_from_iter=10,
                       densification_interval=10, opacity_reset_interval=30, densify_until_iter=50,
                       optimizer_type="sparse_adam")
    problem = ex.make_problem(dev, P=1500, W=128, H=80, n_views=4)
    whole = ex.make_model(problem, opt, dataset)
    sizes = []
    ex.train(whole, problem, opt, 0, 2 * K, dataset=dataset, on_iteration=lambda it, m: sizes.append(m._xyz.shape[0]))
    assert len(set(sizes)) > 1, "the window must hold a densification that changes the model"
    first = ex.make_model(problem, opt, dataset)
    ex.train(first, problem, opt, 0, K, dataset=dataset)
    path = str(tmp_path / f"chkpnt{K}.pth")
    save_checkpoint(first, K, path)
    del first
    resumed = ex.make_model(problem, opt, dataset)               # a fresh model, as train.py:37-42
    assert load_checkpoint(resumed, path, opt) == K
    assert type(resumed.optimizer) is optim.SparseGaussianAdam and type(whole.optimizer) is optim.SparseGaussianAdam
    ex.train(resumed, problem, opt, K, 2 * K, dataset=dataset)
    assert _same_params(_params(whole), _params(resumed))
    for ga, gb in zip(whole.optimizer.param_groups, resumed.optimizer.param_groups):
        sa, sb = whole.optimizer.state.get(ga["params"][0], {}), resumed.optimizer.state.get(gb["params"][0], {})
        assert ga["lr"] == gb["lr"] and ("step" in sa) == ("step" in sb)
        if "step" in sa:
            assert float(sa["step"]) == float(sb["step"])
    for k in ("xyz_gradient_accum", "denom", "max_radii2D"):
        assert torch.equal(getattr(whole, k), getattr(resumed, k)), k
