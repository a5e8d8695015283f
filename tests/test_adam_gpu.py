"""Adam / AdamW (csrc/cl_optim.hip: dlka_optim_adam_step; deformablelka_amd/optim.py) on the MI355X: the cases and bounds of tests/test_adam_emu.py
(tests/adam_cases.py, tests/adam_ref.py — counts of 2^-24 per term: exp_avg 10 on |m| + |g_c|; exp_avg_sq 3 on beta2 v and 14 on
(1 - beta2) g_c^2; parameter 4 on |p| (1 + lr wd) and 10 on step_size |m| / denom plus the carried-in bounds; torch's CPU float32 step held
to the same), and the two trainer hooks that need a device: the eager run_iteration and the captured iteration whose learning rate changes
between replays and whose step counts advance on the device.  Reached on the MI355X, as a fraction of the bound: norm 0.45, exp_avg 0.10, exp_avg_sq 0.69, max_exp_avg_sq 0.68, parameter 0.53 (torch's CPU step: exp_avg 0.09, exp_avg_sq 0.83,
max_exp_avg_sq 0.83, parameter 0.53); the emulator's figures."""
import pytest
import torch

from tests import adam_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
LIST_NAMES = [n for n in C.LISTS if n != "aligned_twin"]


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("reached, error / bound:", C.REACHED)


@pytest.mark.parametrize("hyper", list(C.HYPER))
@pytest.mark.parametrize("name", LIST_NAMES)
def test_three_steps_within_the_rounding_bounds(name, hyper):
    C.run_list(name, hyper, DEV)


@pytest.mark.parametrize("hyper", ["trainer3d_adam", "lka2d_adamw"])
@pytest.mark.parametrize("scale", [100.0, 1e-3], ids=["far_above_max_norm", "far_below_max_norm"])
def test_both_sides_of_the_clamp_and_tiny_second_moments(scale, hyper):
    C.run_list("sizes", hyper, DEV, grad_scale=scale)


def test_two_and_three_groups_with_different_learning_rates():
    C.run_list("sizes", "trainer3d_adam", DEV, lrs=(0.1, 0.025))
    C.run_list("cut_plus_1", "lka2d_adamw", DEV, lrs=(0.1, 0.05, 0.2))


def test_five_steps_under_the_poly_schedule():
    from deformablelka_amd import optim
    C.run_list("sizes", "lka2d_adamw", DEV, steps=5, schedule=lambda k: optim.poly_lr(k, 5, C.LR))
    C.run_list("off_all", "trainer3d_adam", DEV, steps=5, schedule=lambda k: optim.poly_lr(k, 5, C.LR))


def test_two_runs_and_the_shifted_twin_give_the_same_bits():
    for hyper in ("trainer3d_adam", "lka2d_adamw"):
        a, b = C.run_list("off_all", hyper, DEV), C.run_list("off_all", hyper, DEV)
        C.same_bits(a, b)
        C.same_bits(a, C.run_list("aligned_twin", hyper, DEV))
    C.same_bits(C.run_list("sizes", "trainer3d_adam", DEV), C.run_list("sizes", "trainer3d_adam", DEV))


@pytest.mark.parametrize("hyper", ["trainer3d_adam", "lka2d_adamw"], ids=["clip", "no_clip"])
@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_nonfinite_gradient_propagates_as_in_torch(bad, hyper):
    C.check_nonfinite(bad, hyper, DEV)


@pytest.mark.parametrize("hyper", ["trainer3d_adam", "lka2d_adamw"])
def test_state_dict_from_torch(hyper):
    C.check_state_dict_torch_to_hip(hyper, DEV)


@pytest.mark.parametrize("hyper", ["trainer3d_adam", "lka2d_adamw"])
def test_state_dict_into_torch(hyper):
    C.check_state_dict_hip_to_torch(hyper, DEV)


def test_refusals_launch_nothing():
    C.check_refusals(DEV)


def test_not_implemented_arguments_are_named():
    C.check_not_implemented(DEV)


def test_interface_and_learning_rate_uploads():
    C.check_interface(DEV)


def test_reduce_lr_on_plateau_drives_the_rate_through_param_groups():
    C.check_reduce_lr_on_plateau(DEV)


def _batch():
    torch.manual_seed(0)
    return torch.randn(2, 1, 16, 32, 32, device=DEV), torch.randint(0, 3, (2, 16, 32, 32), device=DEV)


def _twin_nets(n):
    nets = [C.lite_net().to(DEV).train() for _ in range(n)]
    for net in nets[1:]:
        net.load_state_dict(nets[0].state_dict())
    return nets


def test_eager_trainer_iteration_follows_torch_adam():
    """run_iteration with initialize_optimizer(fused="hip", algorithm="adam") against the same net under torch.optim.Adam(3e-4,
    weight_decay=3e-5, amsgrad=True): the losses of three iterations (each depends on the updates before it) agree within 2e-2 relative,
    the criterion of tests/test_optim_gpu.py."""
    from deformablelka_amd import _lib, optim, training
    x, tgt = _batch()
    hip_net, ref_net = _twin_nets(2)
    hip_opt = training.initialize_optimizer(hip_net, fused="hip", algorithm="adam")
    ref_opt = torch.optim.Adam(ref_net.parameters(), 3e-4, weight_decay=3e-5, amsgrad=True)
    assert type(hip_opt) is optim.Adam
    before = _lib.get_lib().dlka_optim_launch_count()
    a = [float(training.run_iteration(hip_net, hip_opt, x, tgt)) for _ in range(3)]
    b = [float(training.run_iteration(ref_net, ref_opt, x, tgt)) for _ in range(3)]
    print("losses hip", a, "torch", b)
    assert _lib.get_lib().dlka_optim_launch_count() > before and hip_opt.last_grad_norm is not None
    assert all(abs(u - v) <= 2e-2 * abs(v) for u, v in zip(a, b)), (a, b)
    assert a[0] != a[2]
    assert all(float(hip_opt.state[p]["step"]) == 3.0 for p in hip_net.parameters() if p in hip_opt.state)


def test_captured_iteration_follows_the_rate_and_counts_its_replays():
    """GraphedIteration with optim.AdamW: replay k runs with the rate eager step k used and reaches the eager run's parameters (the criterion
    of tests/test_optim_gpu.py); the step counts after k replays are warm-up + k; a replay at lr = 0 with weight_decay = 0 leaves every
    parameter bit-identical while exp_avg still moves."""
    from deformablelka_amd import optim, training
    x, tgt = _batch()
    eager_net, graph_net = _twin_nets(2)
    eager_opt = optim.AdamW(eager_net.parameters(), 1e-3, weight_decay=0.0)   # (the decay is a launch argument: the capture holds it)
    graph_opt = optim.AdamW(graph_net.parameters(), 1e-3, weight_decay=0.0)
    rates = [optim.poly_lr(k, 8, 1e-3) for k in range(3, 6)]
    eager = []
    for k in range(6):   # three iterations at the initial rate (the capture's warm-up), then the schedule
        if k >= 3:
            eager_opt.param_groups[0]["lr"] = rates[k - 3]
        eager.append(float(training.run_iteration(eager_net, eager_opt, x, tgt)))
    it = training.GraphedIteration(graph_net, graph_opt, x, tgt, warmup=3)
    stepped = [p for p in graph_net.parameters() if p in graph_opt.state]
    assert stepped and all(float(graph_opt.state[p]["step"]) == 3.0 for p in stepped)
    graphed = []
    for k, r in enumerate(rates):
        graph_opt.param_groups[0]["lr"] = r
        graphed.append(float(it()))
        assert graph_opt.lr_tensor.cpu().tolist() == [float(torch.tensor(r, dtype=torch.float32))]
        assert all(float(graph_opt.state[p]["step"]) == 4.0 + k for p in stepped)
    print("losses eager", eager[3:], "graphed", graphed)
    assert all(abs(u - v) <= 2e-2 * abs(u) for u, v in zip(eager[3:], graphed)), (eager, graphed)
    for p, q in zip(eager_net.parameters(), graph_net.parameters()):   # the same rates reached the same parameters
        assert (p - q).abs().max() <= 2e-2 * p.abs().max().clamp_min(1e-3)
    assert all(float(eager_opt.state[p]["step"]) == 6.0 for p in eager_net.parameters() if p in eager_opt.state)
    graph_opt.param_groups[0]["lr"] = 0.0
    held = [p.detach().clone() for p in graph_net.parameters()]
    avg = [graph_opt.state[p]["exp_avg"].clone() for p in stepped]
    it()
    assert all(torch.equal(p.detach(), h) for p, h in zip(graph_net.parameters(), held))
    assert any(not torch.equal(graph_opt.state[p]["exp_avg"], a) for p, a in zip(stepped, avg))
    assert all(float(graph_opt.state[p]["step"]) == 7.0 for p in stepped)
