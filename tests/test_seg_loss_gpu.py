"""The fused Dice + cross-entropy losses on the MI355X: the fixture cases of tests/golden/reference_losses.pt, the three head shapes D_LKA_Former
returns for a 64x128x128 patch (from tests/golden/reference_nets.pt) against the float64 restatement, reproducibility, launch counts, the
online-evaluation counts, and the trainer iteration (eager, captured in a hipGraph, and on the real net).  Tolerances: DESIGN.md §"Tolerances" —
loss and Dice coefficients 1e-4 absolute, gradients 1e-3 of max|grad| per head, bf16 logits 2e-2.  The errors reached are recorded in DESIGN.md
§"Segmentation losses"."""
import os

import pytest
import torch

from tests import seg_loss_cases as C
from tests import seg_loss_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FX = C.load_fixture()
NAMES = list(FX["cases"].keys())


@pytest.fixture(scope="module", autouse=True)
def hip_backend():
    from deformablelka_amd import _lib
    _lib._set_backend_for_tests(None)
    assert torch.cuda.is_available()
    _lib.get_lib()
    yield


@pytest.mark.parametrize("label_dtype", [torch.float32, torch.int64], ids=["labels_f32", "labels_i64"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", NAMES)
def test_fixture_case(name, dtype, label_dtype):
    C.check_case(name, FX["cases"][name], DEV, dtype, label_dtype)


@pytest.mark.parametrize("label_dtype", [torch.float32, torch.int64], ids=["labels_f32", "labels_i64"])
def test_vector_shape_at_unaligned_pointers(label_dtype):
    """A shape whose aligned twin takes the 16-byte kernels (K = 4, N % 4 == 0), logits and labels one element off 16-byte alignment: the scalar kernels."""
    C.check_unaligned_vector_shape(DEV, label_dtype)


@pytest.mark.parametrize("name", NAMES)
def test_online_eval_counts_fixture(name):
    C.check_counts(FX["cases"][name], DEV)


def real_heads(seed=0, B=2):
    """Logits and labels at the net's own head shapes; every class is present in every head's labels."""
    nets = torch.load(os.path.join(os.path.dirname(C.FIXTURE), "reference_nets.pt"), weights_only=False)
    shapes = [tuple(s) for s in nets["D_LKA_Former_plumbing"]["out_shapes"]]
    gen = torch.Generator().manual_seed(seed)
    xs, ys = [], []
    for s in shapes:
        K, spatial = s[1], s[2:]
        xs.append(torch.randn((B, K) + spatial, generator=gen) * 2.0)
        y = torch.randint(0, K, (B, 1) + spatial, generator=gen).float()
        y.view(B, -1)[:, :K] = torch.arange(K, dtype=torch.float32)
        ys.append(y)
    return xs, ys


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_real_head_shapes_against_the_float64_restatement(dtype):
    from deformablelka_amd import training
    xs, ys = real_heads()
    assert [tuple(x.shape[2:]) for x in xs][0] == (64, 128, 128) and len(xs) == 3
    fn = training.initialize_loss(num_heads=len(xs))
    case = dict(kind="nnunet", logits=xs, labels=ys, dice_kw={"batch_dice": True, "smooth": 1e-5, "do_bg": False}, weights=fn.weight_factors,
                weight_ce=1, weight_dice=1)
    xd = [x.to(DEV).double().requires_grad_(True) for x in xs]    # the restatement in float64 on the device
    yd = [y.to(DEV) for y in ys]
    ref = R.multiple_output(xd, yd, fn.weight_factors, **case["dice_kw"])
    ref.backward()
    case["loss"] = ref.detach().cpu()
    case["grads"] = [x.grad.cpu() for x in xd]
    case["dc"] = [R.soft_dice_coefficients(x.detach(), y, True, 1e-5).cpu() for x, y in zip(xd, yd)]
    del xd, ref
    C.check_case("real_heads", case, DEV, dtype)


def test_forward_and_backward_are_bitwise_reproducible():
    xs, ys = real_heads(1)
    case = dict(kind="nnunet", logits=xs[1:], labels=ys[1:], dice_kw={"batch_dice": True, "smooth": 1e-5, "do_bg": False}, weights=[0.6, 0.4],
                weight_ce=1, weight_dice=1)
    a, b = C.run_fused(case, DEV), C.run_fused(case, DEV)
    assert torch.equal(a[0], b[0])
    for ga, gb, da, db in zip(a[1], b[1], a[2], b[2]):
        assert torch.equal(ga, gb) and torch.equal(da, db)


def test_launch_counts():
    """At most two launches per head forward and one per head backward."""
    from deformablelka_amd import ops, training
    xs, ys = real_heads(2)
    xs = [x[:, :, :8].contiguous().to(DEV).requires_grad_(True) for x in xs]
    ys = [y[:, :, :8].contiguous().to(DEV) for y in ys]
    fn = training.initialize_loss(num_heads=3)
    n0 = ops.seg_loss_launch_count()
    loss = fn(xs, ys)
    n1 = ops.seg_loss_launch_count()
    loss.backward()
    torch.cuda.synchronize()
    n2 = ops.seg_loss_launch_count()
    assert 3 <= n1 - n0 <= 2 * 3 and n2 - n1 == 3, (n0, n1, n2)


def test_online_eval_counts_at_the_real_heads():
    from deformablelka_amd import losses
    xs, ys = real_heads(3)
    for x, y in zip(xs, ys):
        x, y = x.to(DEV), y.to(DEV)
        got = torch.stack(losses.online_eval_counts(x, y))
        assert torch.equal(got, R.eval_counts(x, y))
        assert torch.equal(torch.stack(losses.online_eval_counts(x.bfloat16(), y.long())), R.eval_counts(x.bfloat16(), y))


class ThreeHeads(torch.nn.Module):
    """A small stand-in for the net: three conv heads at full, 1/2 and 1/4 resolution."""

    def __init__(self, K=5):
        super().__init__()
        self.stem = torch.nn.Conv3d(1, 8, 3, padding=1)
        self.heads = torch.nn.ModuleList([torch.nn.Conv3d(8, K, 1) for _ in range(3)])

    def forward(self, x):
        f = torch.relu(self.stem(x))
        return [self.heads[0](f), self.heads[1](torch.nn.functional.avg_pool3d(f, 2)), self.heads[2](torch.nn.functional.avg_pool3d(f, 4))]


def test_graphed_iteration_with_the_new_loss_equals_the_eager_step():
    from deformablelka_amd import training
    torch.manual_seed(0)
    x = torch.randn(2, 1, 8, 16, 16, device=DEV)
    tgt = torch.randint(0, 5, (2, 1, 8, 16, 16), device=DEV).float()
    nets = []
    for _ in range(2):
        torch.manual_seed(1)
        net = ThreeHeads().to(DEV)
        nets.append((net, training.initialize_optimizer(net, initial_lr=1e-2)))
    fn = training.initialize_loss()
    eager = [training.run_iteration(nets[0][0], nets[0][1], x, tgt, loss_fn=fn) for _ in range(5)]
    it = training.GraphedIteration(nets[1][0], nets[1][1], x, tgt, loss_fn=fn, warmup=3)
    graphed = [it() for _ in range(2)]
    print("eager", [float(v) for v in eager], "graphed", [float(v) for v in graphed])
    # The replay runs the kernels the eager step runs, on the same inputs.  The fused loss is bitwise reproducible; the stock convolution
    # weight-gradient kernels of the stand-in net may add their partial sums in a different order from one run to the next (fp32, reductions over
    # 4096 voxels: a few 1e-7 relative per step), so the comparison allows 1e-5 relative on the loss and on every parameter.
    for a, b in zip(eager[3:], graphed):
        assert abs(float(a) - float(b)) <= 1e-5 * abs(float(a)), (eager, graphed)
    for p, q in zip(nets[0][0].parameters(), nets[1][0].parameters()):
        assert float((p - q).abs().max()) <= 1e-5 * float(p.abs().max())


def test_run_iteration_of_the_real_net_with_the_new_loss():
    from deformablelka_amd import training
    torch.manual_seed(0)
    net = training.initialize_network(1, 14, (64, 128, 128), device=DEV).train()
    opt = training.initialize_optimizer(net, initial_lr=1e-3)
    x = torch.randn(2, 1, 64, 128, 128, device=DEV)
    tgt = torch.randint(0, 14, (2, 1, 64, 128, 128), device=DEV).float()
    loss = training.run_iteration(net, opt, x, tgt, loss_fn=training.initialize_loss())
    assert bool(torch.isfinite(loss)), loss
    assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in net.parameters())
