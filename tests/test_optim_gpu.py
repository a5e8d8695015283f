"""The optimizer step (csrc/cl_optim.hip, deformablelka_amd/optim.py) on the MI355X: the cases and bounds of tests/test_optim_emu.py
(tests/optim_cases.py: norm 2^-23 relative; momentum buffer 8 * 2^-24 (m |buf| + |g_c| + wd |p|); parameter
16 * 2^-24 (|p| + lr (1 + m) (|g_c| + wd |p| + m |buf|)), torch's CPU float32 step held to the same), and the two trainer hooks that need a
device: the eager run_iteration and the captured iteration whose learning rate changes between replays.  Reached on the MI355X, as a fraction
of the bound: norm 0.45, buffer 0.39, parameter 0.21 — the emulator's figures (the same bits); torch's CPU step: buffer 0.49, parameter 0.19."""
import pytest
import torch

from tests import optim_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
LIST_NAMES = [n for n in C.LISTS if n != "aligned_twin"]


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("reached, error / bound:", C.REACHED)


@pytest.mark.parametrize("hyper", list(C.HYPER))
@pytest.mark.parametrize("name", LIST_NAMES)
def test_two_steps_within_the_rounding_bounds(name, hyper):
    C.run_list(name, hyper, DEV)


@pytest.mark.parametrize("scale", [100.0, 1e-3], ids=["far_above_max_norm", "far_below_max_norm"])
def test_both_sides_of_the_clamp(scale):
    C.run_list("sizes", "synapse3d", DEV, grad_scale=scale)


def test_two_groups_with_different_learning_rates():
    C.run_list("sizes", "synapse3d", DEV, lrs=(0.1, 0.025))
    C.run_list("cut_plus_1", "maxvit2d", DEV, lrs=(0.1, 0.05, 0.2))


def test_five_steps_under_the_poly_schedule():
    from deformablelka_amd import optim
    C.run_list("sizes", "synapse3d", DEV, steps=5, schedule=lambda k: optim.poly_lr(k, 5, C.LR))
    C.run_list("off_all", "maxvit2d", DEV, steps=5, schedule=lambda k: optim.poly_lr(k, 5, C.LR))


def test_two_runs_and_the_shifted_twin_give_the_same_bits():
    a, b = C.run_list("off_all", "synapse3d", DEV), C.run_list("off_all", "synapse3d", DEV)
    C.same_bits(a, b)
    C.same_bits(a, C.run_list("aligned_twin", "synapse3d", DEV))
    C.same_bits(C.run_list("sizes", "synapse3d", DEV), C.run_list("sizes", "synapse3d", DEV))


@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_nonfinite_gradient_propagates_as_in_torch(bad):
    C.check_nonfinite(bad, DEV)


def test_state_dict_from_torch():
    C.check_state_dict_torch_to_hip(DEV)


def test_state_dict_into_torch():
    C.check_state_dict_hip_to_torch(DEV)


@pytest.mark.parametrize("scale", [1.0, 1e-3], ids=["clipped", "not_clipped"])
@pytest.mark.parametrize("name", ["sizes", "cut_plus_1", "off_grad"])
def test_clip_grad_norm_scales_in_place_and_returns_the_norm(name, scale):
    C.check_clip_grad_norm(name, DEV, scale)


def test_refusals_launch_nothing():
    C.check_refusals(DEV)


def test_not_implemented_arguments_are_named():
    C.check_not_implemented(DEV)


def test_interface_and_learning_rate_uploads():
    C.check_interface(DEV)


def _nets(n, fused):
    from deformablelka_amd import training
    out = []
    for f in fused[:n]:
        net = C.lite_net().to(DEV).train()
        out.append((net, training.initialize_optimizer(net, initial_lr=1e-2, fused=f)))
    for net, _ in out[1:]:
        net.load_state_dict(out[0][0].state_dict())
    return out


def _batch():
    torch.manual_seed(0)
    return torch.randn(2, 1, 16, 32, 32, device=DEV), torch.randint(0, 3, (2, 16, 32, 32), device=DEV)


def test_eager_trainer_iteration_follows_the_torch_optimizer():
    """run_iteration with initialize_optimizer(fused="hip") against the same net stepped with torch's fused SGD: the losses of three iterations
    (each depends on the updates before it) agree as test_graphed_trainer_iteration_follows_the_eager_one requires, 2e-2 relative."""
    from deformablelka_amd import _lib, optim, training
    x, tgt = _batch()
    (hip_net, hip_opt), (ref_net, ref_opt) = _nets(2, ["hip", True])
    assert isinstance(hip_opt, optim.SGD)
    before = _lib.get_lib().dlka_optim_launch_count()
    a = [float(training.run_iteration(hip_net, hip_opt, x, tgt)) for _ in range(3)]
    b = [float(training.run_iteration(ref_net, ref_opt, x, tgt)) for _ in range(3)]
    print("losses hip", a, "torch", b)
    assert _lib.get_lib().dlka_optim_launch_count() > before and hip_opt.last_grad_norm is not None
    assert all(abs(u - v) <= 2e-2 * abs(v) for u, v in zip(a, b)), (a, b)
    assert a[0] != a[2]


def test_captured_iteration_follows_a_changing_learning_rate():
    """GraphedIteration with the HIP optimizer: replay k runs with the rate eager step k used (set between replays, uploaded in front of the
    replay); a replay at lr = 0 leaves every parameter bit-identical; torch's optimizer still raises on a changed rate."""
    from deformablelka_amd import optim, training
    x, tgt = _batch()
    (eager_net, eager_opt), (graph_net, graph_opt), (torch_net, torch_opt) = _nets(3, ["hip", "hip", True])
    rates = [optim.poly_lr(k, 8, 1e-2) for k in range(3, 6)]
    eager = []
    for k in range(6):   # three iterations at the initial rate (the capture's warm-up), then the schedule
        if k >= 3:
            eager_opt.param_groups[0]["lr"] = rates[k - 3]
        eager.append(float(training.run_iteration(eager_net, eager_opt, x, tgt)))
    it = training.GraphedIteration(graph_net, graph_opt, x, tgt, warmup=3)
    graphed = []
    for r in rates:
        graph_opt.param_groups[0]["lr"] = r
        graphed.append(float(it()))
        assert graph_opt.lr_tensor.cpu().tolist() == [float(torch.tensor(r, dtype=torch.float32))]
    print("losses eager", eager[3:], "graphed", graphed)
    assert all(abs(u - v) <= 2e-2 * abs(u) for u, v in zip(eager[3:], graphed)), (eager, graphed)
    for p, q in zip(eager_net.parameters(), graph_net.parameters()):   # the same rates reached the same parameters
        assert (p - q).abs().max() <= 2e-2 * p.abs().max().clamp_min(1e-3)
    graph_opt.param_groups[0]["lr"] = 0.0
    held = [p.detach().clone() for p in graph_net.parameters()]
    it()
    assert all(torch.equal(p.detach(), h) for p, h in zip(graph_net.parameters(), held))
    graph_opt.param_groups[0]["lr"] = 1e-2   # back to the rate the capture saw: uploaded again all the same
    it()
    assert graph_opt.lr_tensor.cpu().tolist() == [float(torch.tensor(1e-2, dtype=torch.float32))]
    assert any(not torch.equal(p.detach(), h) for p, h in zip(graph_net.parameters(), held))
    it2 = training.GraphedIteration(torch_net, torch_opt, x, tgt, warmup=3)
    it2()
    torch_opt.param_groups[0]["lr"] = 5e-3
    with pytest.raises(RuntimeError, match="learning rate changed"):
        it2()
