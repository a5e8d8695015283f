"""Adam / AdamW (csrc/cl_optim.hip: dlka_optim_adam_step; deformablelka_amd/optim.py) on the wavefront emulator: three checked steps per case
against the float64 restatement under the rounding bounds of tests/adam_ref.py — counts of 2^-24 per term: exp_avg 10 on |m| + |g_c|;
exp_avg_sq 3 on beta2 v and 14 on (1 - beta2) g_c^2 (max_exp_avg_sq the same); parameter 4 on |p| (1 + lr wd) and 10 on
step_size |m| / denom, plus the bounds of the new exp_avg and exp_avg_sq carried through the quotient — with torch's CPU float32 Adam / AdamW
step from the same state held to the same bounds in every case, and the device-side step counts checked after every step.
Reached on the emulator, as a fraction of the bound: norm 0.45, exp_avg 0.10, exp_avg_sq 0.69, max_exp_avg_sq 0.68, parameter 0.53 (torch's CPU step: exp_avg 0.09, exp_avg_sq 0.83,
max_exp_avg_sq 0.83, parameter 0.53); the MI355X reaches the same figures (tests/test_adam_gpu.py)."""
import pytest
import torch

from tests import adam_cases as C


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
def test_three_steps_within_the_rounding_bounds(name, hyper):
    C.run_list(name, hyper, "cpu")


@pytest.mark.parametrize("hyper", ["trainer3d_adam", "lka2d_adamw"])
@pytest.mark.parametrize("scale", [100.0, 1e-3], ids=["far_above_max_norm", "far_below_max_norm"])
def test_both_sides_of_the_clamp_and_tiny_second_moments(scale, hyper):
    C.run_list("sizes", hyper, "cpu", grad_scale=scale)


def test_two_and_three_groups_with_different_learning_rates():
    C.run_list("sizes", "trainer3d_adam", "cpu", lrs=(0.1, 0.025))
    C.run_list("cut_plus_1", "lka2d_adamw", "cpu", lrs=(0.1, 0.05, 0.2))


def test_five_steps_under_the_poly_schedule():
    from deformablelka_amd import optim
    C.run_list("sizes", "lka2d_adamw", "cpu", steps=5, schedule=lambda k: optim.poly_lr(k, 5, C.LR))
    C.run_list("off_all", "trainer3d_adam", "cpu", steps=5, schedule=lambda k: optim.poly_lr(k, 5, C.LR))


def test_two_runs_and_the_shifted_twin_give_the_same_bits(monkeypatch):
    monkeypatch.setenv("HIPEMU_THREADS", "1")
    for hyper in ("trainer3d_adam", "lka2d_adamw"):
        a, b = C.run_list("off_all", hyper, "cpu"), C.run_list("off_all", hyper, "cpu")
        C.same_bits(a, b)
        C.same_bits(a, C.run_list("aligned_twin", hyper, "cpu"))
    C.same_bits(C.run_list("sizes", "trainer3d_adam", "cpu"), C.run_list("sizes", "trainer3d_adam", "cpu"))


@pytest.mark.parametrize("hyper", ["trainer3d_adam", "lka2d_adamw"], ids=["clip", "no_clip"])
@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_nonfinite_gradient_propagates_as_in_torch(bad, hyper):
    C.check_nonfinite(bad, hyper, "cpu")


@pytest.mark.parametrize("hyper", ["trainer3d_adam", "lka2d_adamw"])
def test_state_dict_from_torch(hyper):
    C.check_state_dict_torch_to_hip(hyper, "cpu")


@pytest.mark.parametrize("hyper", ["trainer3d_adam", "lka2d_adamw"])
def test_state_dict_into_torch(hyper):
    C.check_state_dict_hip_to_torch(hyper, "cpu")


def test_refusals_launch_nothing():
    C.check_refusals("cpu")


def test_not_implemented_arguments_are_named():
    C.check_not_implemented("cpu")


def test_interface_and_learning_rate_uploads():
    C.check_interface("cpu")


def test_reduce_lr_on_plateau_drives_the_rate_through_param_groups():
    C.check_reduce_lr_on_plateau("cpu")


def test_trainer_constructor_rows():
    """initialize_optimizer(fused="hip", algorithm=...) builds the other trainers' rows; the default is the SGD row as before."""
    from deformablelka_amd import optim, training
    net = torch.nn.Linear(5, 3)
    opt = training.initialize_optimizer(net, fused="hip", algorithm="adam")
    g = opt.param_groups[0]
    assert type(opt) is optim.Adam and (g["lr"], g["weight_decay"], g["amsgrad"], g["betas"], g["decoupled_weight_decay"]) == (3e-4, 3e-5, True, (0.9, 0.999), False)
    opt = training.initialize_optimizer(net, fused="hip", algorithm="adamw")
    g = opt.param_groups[0]
    assert type(opt) is optim.AdamW and (g["lr"], g["weight_decay"], g["amsgrad"], g["decoupled_weight_decay"]) == (0.05, 1e-4, False, True)
    assert training.initialize_optimizer(net, 1e-3, 0.0, fused="hip", algorithm="adamw").param_groups[0]["weight_decay"] == 0.0
    opt = training.initialize_optimizer(net, fused="hip")
    g = opt.param_groups[0]
    assert type(opt) is optim.SGD and (g["lr"], g["momentum"], g["nesterov"], g["weight_decay"]) == (1e-2, 0.99, True, 3e-5)
    g = training.initialize_optimizer(net, fused=False).param_groups[0]
    assert (g["lr"], g["weight_decay"]) == (1e-2, 3e-5)
    for kw in (dict(fused="hip", algorithm="rmsprop"), dict(algorithm="adam"), dict(fused=True, algorithm="adamw")):
        with pytest.raises(ValueError, match="algorithm"):
            training.initialize_optimizer(net, **kw)
    x, y = torch.randn(4, 5) * 50, torch.randint(0, 3, (4,))
    ref = torch.nn.Linear(5, 3)
    ref.load_state_dict(net.state_dict())
    opt = training.initialize_optimizer(net, fused="hip", algorithm="adam")
    ropt = torch.optim.Adam(ref.parameters(), 3e-4, weight_decay=3e-5, amsgrad=True)
    for _ in range(2):
        a = training.run_iteration(net, opt, x, y, loss_fn=torch.nn.functional.cross_entropy, clip_norm=0.5)
        b = training.run_iteration(ref, ropt, x, y, loss_fn=torch.nn.functional.cross_entropy, clip_norm=0.5)
        assert torch.allclose(a, b, rtol=1e-5)
    assert float(opt.last_grad_norm) > 0.5
    for p, q in zip(net.parameters(), ref.parameters()):
        assert torch.allclose(p, q, rtol=1e-5, atol=1e-6)
