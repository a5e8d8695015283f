"""The optimizer step (csrc/cl_optim.hip, deformablelka_amd/optim.py) on the wavefront emulator: clip + SGD against the float64 restatement
(tests/optim_ref.py) under bounds derived from fp32 rounding (tests/optim_cases.py) — norm 2^-23 relative; momentum buffer
8 * 2^-24 (m |buf| + |g_c| + wd |p|); parameter 16 * 2^-24 (|p| + lr (1 + m) (|g_c| + wd |p| + m |buf|)) — with torch's CPU float32 step held to the
same bounds in every case.  Reached on the emulator, as a fraction of the bound: norm 0.45, buffer 0.39, parameter 0.21 (torch's CPU step:
buffer 0.49, parameter 0.19); the MI355X reaches the same figures (tests/test_optim_gpu.py)."""
import pytest
import torch

from tests import optim_cases as C


@pytest.fixture(scope="module", autouse=True)
def emu_backend():
    from deformablelka_amd import _lib
    from tests import emu
    _lib._set_backend_for_tests(emu.load())
    yield
    _lib._set_backend_for_tests(None)
    print("reached, error / bound:", C.REACHED)


LIST_NAMES = [n for n in C.LISTS if n != "aligned_twin"]


@pytest.mark.parametrize("hyper", list(C.HYPER))
@pytest.mark.parametrize("name", LIST_NAMES)
def test_two_steps_within_the_rounding_bounds(name, hyper):
    C.run_list(name, hyper, "cpu")


@pytest.mark.parametrize("scale", [100.0, 1e-3], ids=["far_above_max_norm", "far_below_max_norm"])
def test_both_sides_of_the_clamp(scale):
    C.run_list("sizes", "synapse3d", "cpu", grad_scale=scale)


def test_two_groups_with_different_learning_rates():
    C.run_list("sizes", "synapse3d", "cpu", lrs=(0.1, 0.025))
    C.run_list("cut_plus_1", "maxvit2d", "cpu", lrs=(0.1, 0.05, 0.2))


def test_five_steps_under_the_poly_schedule():
    from deformablelka_amd import optim
    C.run_list("sizes", "synapse3d", "cpu", steps=5, schedule=lambda k: optim.poly_lr(k, 5, C.LR))
    C.run_list("off_all", "maxvit2d", "cpu", steps=5, schedule=lambda k: optim.poly_lr(k, 5, C.LR))


def test_two_runs_and_the_shifted_twin_give_the_same_bits(monkeypatch):
    monkeypatch.setenv("HIPEMU_THREADS", "1")
    a, b = C.run_list("off_all", "synapse3d", "cpu"), C.run_list("off_all", "synapse3d", "cpu")
    C.same_bits(a, b)
    C.same_bits(a, C.run_list("aligned_twin", "synapse3d", "cpu"))
    C.same_bits(C.run_list("sizes", "synapse3d", "cpu"), C.run_list("sizes", "synapse3d", "cpu"))


@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_nonfinite_gradient_propagates_as_in_torch(bad):
    C.check_nonfinite(bad, "cpu")


def test_state_dict_from_torch():
    C.check_state_dict_torch_to_hip("cpu")


def test_state_dict_into_torch():
    C.check_state_dict_hip_to_torch("cpu")


@pytest.mark.parametrize("scale", [1.0, 1e-3], ids=["clipped", "not_clipped"])
@pytest.mark.parametrize("name", ["sizes", "cut_plus_1", "off_grad"])
def test_clip_grad_norm_scales_in_place_and_returns_the_norm(name, scale):
    C.check_clip_grad_norm(name, "cpu", scale)


def test_refusals_launch_nothing():
    C.check_refusals("cpu")


def test_not_implemented_arguments_are_named():
    C.check_not_implemented("cpu")


def test_interface_and_learning_rate_uploads():
    C.check_interface("cpu")


def test_trainer_hooks_select_the_hip_optimizer():
    """initialize_optimizer(fused="hip") builds the trainer's configuration; run_iteration hands the clip norm to step()."""
    from deformablelka_amd import optim, training
    net = torch.nn.Linear(5, 3)
    opt = training.initialize_optimizer(net, initial_lr=0.02, weight_decay=3e-5, fused="hip")
    assert isinstance(opt, optim.SGD)
    g = opt.param_groups[0]
    assert (g["lr"], g["momentum"], g["nesterov"], g["weight_decay"], g["dampening"]) == (0.02, 0.99, True, 3e-5, 0)
    assert type(training.initialize_optimizer(net, fused=False)) is torch.optim.SGD
    with pytest.raises(ValueError, match="fused"):
        training.initialize_optimizer(net, fused="cuda")
    x, y = torch.randn(4, 5) * 50, torch.randint(0, 3, (4,))
    ref = torch.nn.Linear(5, 3)
    ref.load_state_dict(net.state_dict())
    ropt = training.initialize_optimizer(ref, initial_lr=0.02, fused=False)
    for _ in range(2):
        a = training.run_iteration(net, opt, x, y, loss_fn=torch.nn.functional.cross_entropy, clip_norm=0.5)
        b = training.run_iteration(ref, ropt, x, y, loss_fn=torch.nn.functional.cross_entropy, clip_norm=0.5)
        assert torch.allclose(a, b, rtol=1e-5)
    assert float(opt.last_grad_norm) > 0.5
    for p, q in zip(net.parameters(), ref.parameters()):
        assert torch.allclose(p, q, rtol=1e-5, atol=1e-6)
