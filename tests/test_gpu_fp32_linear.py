"""The fp32 Linear path at operator level: the bf16x3 products (ops/gemm.py, csrc/split3.hip) EXACTLY, the weight-split cache behind
them, and the fp32 training step under HIP-graph replay.

A. The three products.  Every operand element is I + J 2^-10 with I in {+-1, +-2, +-3} and J in {-1, 0, 1}, held as fp32.  |J| 2^-10 is
below half a bf16 ulp of every such I (also from below at |I| = 1, where the spacing is 2^-8), so the split is hi = I, lo = J 2^-10 with
no residual (asserted per case with torch's own bf16 rounding).  Every term of hi hi + hi lo + lo hi is a multiple of 2^-10 and the sum
of their magnitudes over a reduction of length K <= 1025 stays below 9 K + 6 K 2^-10 < 2^14: 24 bits, so fp32 accumulation is exact in
ANY order and y, dx, dW, db must EQUAL the float64 value of hi hi^T + hi lo^T + lo hi^T (+ the integer bias / addend).  That value
differs from the full product by exactly (J_a J_b^T) 2^-20 -- asserted too: the inputs do exercise the dropped term.  A lost or doubled
cross term, a wrong column block, a token read twice changes a multiple of 2^-10.  No tolerance anywhere in parts A and B.
Each case asserts its own precondition (`_bf16x3_ok`, a launch census through _lib_spy) so that it cannot fall back unnoticed to
F.linear or the exact-fp32 kernels.

B. `_weight_split` follows the weights: raw-pointer updates and `RT.weight_epoch`, `note_forward`'s rule, FlatAdam.step(), the bound
on `_WSPLIT` -- the rules tests/test_host_logic.py checks with a fake library, here with the real split kernel and product values.

C. The fp32 step under `GraphedTrainStep`: graph equals eager, and an eager evaluation between replays sees the current weights (it
must equal a FRESH model built from the graphed model's state_dict, which has no cache history)."""
import ctypes
import functools

import pytest
import torch

from _lib_spy import spy_on

pytestmark = pytest.mark.gpu
DEV = "cuda"
LO = 2.0 ** -10
SHAPES = [(512, 512), (1024, 256), (256, 1024), (768, 256), (328, 320)]  # (n_out, k_in); 328 x 320: multiples of 8, not of 64, ratio 162
ROWS = [1, 33, 200, 1025]                                                # 1025: three token slices in the weight gradient
CASES = [pytest.param(n, k, r, id=f"{n}x{k}-rows{r}") for n, k in SHAPES for r in ROWS]
CENSUS = ("hs_split_bf16x3", "hs_linear_wgrad", "hs_gelu_split3")


def _G():
    from heal_swin_amd.ops import gemm
    return gemm


@pytest.fixture(scope="module", autouse=True)
def _needs_mm_out_dtype():
    G = _G()
    if G._MM_OUT_DTYPE[0] is None:
        G._probe_mm_out_dtype(torch.device(DEV))
    if G._MM_OUT_DTYPE[0] is False:
        pytest.skip("torch.mm(..., out_dtype=) is missing in this PyTorch build: fp32 products run as exact fp32 GEMMs, there is no bf16x3 path to test")


# ----------------------------------------------------------------------------- operands and float64 references
class Parts:
    """An operand as its two float64 parts: value = i + j 2^-10."""

    def __init__(self, shape, g):
        sign = 2 * torch.randint(0, 2, shape, generator=g, device=DEV) - 1
        self.i = (sign * torch.randint(1, 4, shape, generator=g, device=DEV)).double()
        self.j = torch.randint(-1, 2, shape, generator=g, device=DEV).double()

    @property
    def t(self):
        out = Parts.__new__(Parts)
        out.i, out.j = self.i.t(), self.j.t()
        return out

    def value(self):
        v64 = self.i + self.j * LO
        v = v64.float()
        assert torch.equal(v.double(), v64)
        # what the split kernel must find: hi = I, lo = J 2^-10, nothing left over
        hi = v.to(torch.bfloat16).float()
        lo = (v - hi).to(torch.bfloat16).float()
        assert torch.equal(hi.double(), self.i) and torch.equal(lo.double(), self.j * LO) and torch.equal(hi + lo, v)
        return v


def _ints(shape, g):
    return torch.randint(-3, 4, shape, generator=g, device=DEV).double()


def _x3(a, b):
    """float64 a_hi b_hi^T + a_hi b_lo^T + a_lo b_hi^T of a [m, K], b [n, K]; asserts that the full product differs from it by exactly
    (J_a J_b^T) 2^-20 and that this dropped term is not zero."""
    ref = a.i @ b.i.t() + (a.i @ b.j.t() + a.j @ b.i.t()) * LO
    full = (a.i + a.j * LO) @ (b.i + b.j * LO).t()
    dropped = (a.j @ b.j.t()) * 2.0 ** -20
    assert torch.equal(full - ref, dropped) and bool((dropped != 0).any())
    return ref


def _f32(ref64):
    """The float64 reference as fp32 -- exactly (a multiple of 2^-10 below 2^14)."""
    out = ref64.float()
    assert torch.equal(out.double(), ref64)
    return out


def _refs(x, w, dy):
    """(y, dx, dW, db) of y = x W^T in float64, without bias and addends."""
    return _x3(x, w), _x3(dy, w.t), _x3(dy.t, x.t), (dy.i + dy.j * LO).sum(0)


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(rows, n_out, k_in):
    """Operands of one shape and their exact results, made once and never changed (the tests clone what they hand to an operator)."""
    g = torch.Generator(device=DEV).manual_seed(100000 * rows + 100 * n_out + k_in)
    c = Case()
    c.rows, c.n, c.k = rows, n_out, k_in
    c.xp, c.wp, c.dyp = Parts((rows, k_in), g), Parts((n_out, k_in), g), Parts((rows, n_out), g)
    c.x, c.w, c.dy = c.xp.value(), c.wp.value(), c.dyp.value()
    b, res, dres = _ints((n_out,), g), _ints((rows, n_out), g), _ints((rows, k_in), g)
    c.b, c.res, c.dres = b.float(), res.float(), dres.float()
    y, dx, dw, db = _refs(c.xp, c.wp, c.dyp)
    c.y, c.y_b, c.y_b_res = _f32(y), _f32(y + b), _f32(y + b + res)
    c.dx, c.dx_res = _f32(dx), _f32(dx + dres)
    c.dw, c.db = _f32(dw), _f32(db)
    c.dw64, c.db64 = dw, db
    return c


def _count(called, name):
    return sum(c == name for c in called)


def _other_wgrads(called):
    return [c for c in called if c.startswith("hs_linear_wgrad") and c not in ("hs_linear_wgrad_ld", "hs_linear_wgrad_workspace")]


def _assert_bf16x3(c):
    """The three products of this shape take the bf16x3 form (forward; input gradient: the same ratio with n and k exchanged)."""
    G = _G()
    assert G.FP32_GEMM == "bf16x3" and G._MM_OUT_DTYPE[0] is not False
    assert G._bf16x3_ok(c.x, c.n, c.k) and G._bf16x3_ok(c.dy, c.k, c.n) and c.n % 8 == 0 and c.k % 8 == 0


def _shaped(t, rows):
    """[rows, c], or [2, rows / 2, c] for the 200-row cases: the operators flatten leading dimensions."""
    return t.view(2, rows // 2, t.shape[-1]) if rows == 200 else t


def _pending():
    from heal_swin_amd import _lib
    return int(_lib.lib.hs_reduce_pending(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))


# ----------------------------------------------------------------------------- A. the three products, exactly
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("n_out,k_in,rows", CASES)
def test_linear_forward_and_backward_exact(n_out, k_in, rows, bias, monkeypatch):
    from heal_swin_amd import ops
    c = _case(rows, n_out, k_in)
    _assert_bf16x3(c)
    x = _shaped(c.x.clone(), rows).requires_grad_()
    w = c.w.clone().requires_grad_()
    b = c.b.clone().requires_grad_() if bias else None
    called = spy_on(monkeypatch, CENSUS, [_G()])
    y = ops.linear(x, w, b)
    assert _count(called, "hs_split_bf16x3") == 2, called          # x and the weight
    y.backward(_shaped(c.dy.clone(), rows))
    assert _count(called, "hs_split_bf16x3") == 4, called          # dy (once, for both gradient products) and the transposed weight
    assert _count(called, "hs_linear_wgrad_ld") == 3 and not _other_wgrads(called), called
    assert torch.equal(y.reshape(rows, n_out), c.y_b if bias else c.y), "y"
    assert torch.equal(x.grad.reshape(rows, k_in), c.dx), "dx"
    assert torch.equal(w.grad, c.dw), "dW"
    if bias:
        assert torch.equal(b.grad, c.db), "db"


@pytest.mark.parametrize("n_out,k_in,rows", CASES)
def test_linear_residual_exact(n_out, k_in, rows, monkeypatch):
    """ops.linear_residual in fp32: the integer addend joins the product's result, its gradient is dy itself."""
    from heal_swin_amd import ops
    c = _case(rows, n_out, k_in)
    _assert_bf16x3(c)
    x, w, b = _shaped(c.x.clone(), rows).requires_grad_(), c.w.clone().requires_grad_(), c.b.clone().requires_grad_()
    res = _shaped(c.res.clone(), rows).requires_grad_()
    called = spy_on(monkeypatch, CENSUS, [_G()])
    y = ops.linear_residual(x, w, b, res)
    y.backward(_shaped(c.dy.clone(), rows))
    assert _count(called, "hs_split_bf16x3") == 4 and _count(called, "hs_linear_wgrad_ld") == 3 and not _other_wgrads(called), called
    assert torch.equal(y.reshape(rows, n_out), c.y_b_res), "y"
    assert torch.equal(res.grad.reshape(rows, n_out), c.dy), "dresidual"
    assert torch.equal(x.grad.reshape(rows, k_in), c.dx), "dx"
    assert torch.equal(w.grad, c.dw) and torch.equal(b.grad, c.db), "dW / db"


@pytest.mark.parametrize("n_out,k_in,rows", CASES)
def test_linear_passthrough_exact(n_out, k_in, rows, monkeypatch):
    """ops.linear_passthrough: the gradient of the alias arrives in the Linear's backward and is the `res` addend of the
    input-gradient product (not a separate add over the activation)."""
    from heal_swin_amd import ops
    G = _G()
    c = _case(rows, n_out, k_in)
    _assert_bf16x3(c)
    x, w, b = _shaped(c.x.clone(), rows).requires_grad_(), c.w.clone().requires_grad_(), c.b.clone().requires_grad_()
    called = spy_on(monkeypatch, CENSUS, [G])
    addends, real = [], G._lib_matmul

    def matmul(dy2, w2, res=None):
        addends.append(res)
        return real(dy2, w2, res)
    monkeypatch.setattr(G, "_lib_matmul", matmul)
    y, alias = ops.linear_passthrough(x, w, b)
    assert alias.data_ptr() == x.data_ptr()
    torch.autograd.backward([y, alias], [_shaped(c.dy.clone(), rows), _shaped(c.dres.clone(), rows)])
    assert len(addends) == 1 and addends[0] is not None and torch.equal(addends[0], c.dres)
    assert _count(called, "hs_split_bf16x3") == 4 and _count(called, "hs_linear_wgrad_ld") == 3 and not _other_wgrads(called), called
    assert torch.equal(y.reshape(rows, n_out), c.y_b), "y"
    assert torch.equal(x.grad.reshape(rows, k_in), c.dx_res), "dx"
    assert torch.equal(w.grad, c.dw) and torch.equal(b.grad, c.db), "dW / db"


@pytest.mark.parametrize("n_out,k_in,rows", CASES)
def test_split_stand_ins_equal_the_tensor_forms(n_out, k_in, rows, monkeypatch):
    """`_Split`: an operand that exists only as its [hi | hi | lo] split (what the Mlp hands fc2, and fc1's gradient products) gives
    what the fp32 tensor gives, bit for bit -- and both the exact value."""
    G = _G()
    c = _case(rows, n_out, k_in)
    _assert_bf16x3(c)
    x, w, b, dy = c.x.clone(), c.w.clone(), c.b.clone(), c.dy.clone()
    with torch.no_grad():
        x3, dy3 = G.split3(x, 0), G.split3(dy, 0)
        xs, dys = G._Split(x3, k_in), G._Split(dy3, n_out)
        called = spy_on(monkeypatch, CENSUS, [G])
        y_t, y_s = G._lib_linear(x, w, b), G._lib_linear(xs, w, b)
        assert torch.equal(y_t, c.y_b) and torch.equal(y_s, c.y_b), "_lib_linear"
        assert torch.equal(G._lib_linear(xs, w, None), c.y), "_lib_linear without bias"
        dx_t, dx_s = G._lib_matmul(dy, w), G._lib_matmul(dys, w)
        assert torch.equal(dx_t, c.dx) and torch.equal(dx_s, c.dx), "_lib_matmul"
        assert torch.equal(G._lib_matmul(dys, w, c.dres), c.dx_res) and torch.equal(G._lib_matmul(dy, w, c.dres), c.dx_res), "_lib_matmul + res"
        before = len(called)
        for what, (dy_arg, x_arg, x3_arg) in {"tensors": (dy, x, None), "x as its split": (dy, None, x3),
                                              "both as their splits": (dys, None, x3)}.items():
            dw, db = G._param_grads(dy_arg, x_arg, w, b, True, True, x3=x3_arg)
            assert torch.equal(dw, c.dw) and torch.equal(db, c.db), what
            dw, db = G._param_grads(dy_arg, x_arg, w, None, True, False, x3=x3_arg)
            assert db is None and torch.equal(dw, c.dw), what + ", no bias"
        assert _count(called[before:], "hs_linear_wgrad_ld") == 18 and not _other_wgrads(called), called


@pytest.mark.parametrize("mode", ["deferred", "side_stream"])
@pytest.mark.parametrize("n_out,k_in,rows", CASES)
def test_deposits_into_the_gradient_sink_exact(n_out, k_in, rows, mode, monkeypatch):
    """With a GradBucketAllReduce installed the three weight-gradient products ADD into its buckets; "deferred": the third product's
    slice sum is queued (HS_ACC_DEFER) and the first product of the next pass meets it pending on the same destination; "side_stream":
    ops.AsyncWgrad, nothing is queued, the splits are recorded on the side stream.  Two passes without a flush in between, then
    finish(): the buckets hold preset + 2 x reference exactly (every intermediate value is a partial sum of one pass or preset + one
    pass: below 2^14; the final value is asserted to be exact in fp32)."""
    from heal_swin_amd import ops
    from heal_swin_amd.parallel import GradBucketAllReduce
    G = _G()
    c = _case(rows, n_out, k_in)
    _assert_bf16x3(c)
    w, b = torch.nn.Parameter(c.w.clone()), torch.nn.Parameter(c.b.clone())
    g = torch.Generator(device=DEV).manual_seed(rows + n_out)
    sink = GradBucketAllReduce([w, b], async_wgrad=(mode == "side_stream"))
    try:
        assert ops.RT.grad_sink is sink and (ops.RT.async_wgrad is not None) == (mode == "side_stream")
        assert bool(G._defer_flag(w.device)) == (mode == "deferred")
        assert sum(f.numel() for f in sink.buckets) == w.numel() + b.numel()  # no element that the comparisons below do not see
        called = spy_on(monkeypatch, CENSUS, [G])
        for form in ("tensors", "x as its split"):
            x, dy = c.x.clone(), c.dy.clone()
            x3 = G.split3(x, 0) if form != "tensors" else None
            sink.finish()  # (nothing pending, no pass open)
            pre_w, pre_b = _ints((n_out, k_in), g), _ints((n_out,), g)
            with torch.no_grad():
                w.grad.copy_(pre_w)
                b.grad.copy_(pre_b)
            assert _pending() == 0
            before = len(called)
            for _ in range(2):
                with torch.no_grad():
                    out = G._param_grads(dy, None if x3 is not None else x, w, b, True, True, x3=x3)
                assert out == (None, None)
                assert _pending() == (1 if mode == "deferred" else 0)  # the third product's sum only
            assert _count(called[before:], "hs_linear_wgrad_ld") == 6 and not _other_wgrads(called), called
            sink.finish()
            assert _pending() == 0
            assert torch.equal(w.grad, _f32(pre_w + 2 * c.dw64)), f"{form}: dW bucket"
            assert torch.equal(b.grad, _f32(pre_b + 2 * c.db64)), f"{form}: db bucket"
    finally:
        sink.remove()
    assert ops.RT.grad_sink is None and ops.RT.async_wgrad is None


def _weights(n_out, k_in, count, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    parts = [Parts((n_out, k_in), g) for _ in range(count)]
    return parts, [p.value() for p in parts]


def _raw_write(p, new):
    """Give parameter p the values `new` the way a fused optimizer or a graph replay does: through the storage, `_version` untouched."""
    version = p._version
    torch._foreach_add_([p.data], [new - p.data])  # (the difference of two operands of the class is exact, and so is the sum)
    assert p._version == version and torch.equal(p.data, new)


@pytest.mark.parametrize("n_out,k_in", SHAPES)
def test_input_gradient_takes_the_transposed_split_of_the_current_epoch(n_out, k_in, monkeypatch):
    """The transposed weight split (input-gradient product) is cached like the forward one: after a write through `.data` (`_version`
    stays) and a move of RT.weight_epoch, forward AND input gradient use the new values."""
    from heal_swin_amd import ops
    rows = 33
    c = _case(rows, n_out, k_in)
    _assert_bf16x3(c)
    (_, w2p), (_, w2) = _weights(n_out, k_in, 2, 7 * n_out + k_in)
    y2, dx2, _, _ = _refs(c.xp, w2p, c.dyp)
    w = torch.nn.Parameter(c.w.clone())
    called = spy_on(monkeypatch, CENSUS, [_G()])
    x = c.x.clone().requires_grad_()
    y = ops.linear(x, w)
    y.backward(c.dy.clone())
    assert torch.equal(y, c.y) and torch.equal(x.grad, c.dx)
    version = w._version
    w.data.copy_(w2)
    assert w._version == version
    ops.RT.weight_epoch += 1
    before = len(called)
    x = c.x.clone().requires_grad_()
    y = ops.linear(x, w)
    y.backward(c.dy.clone())
    assert _count(called[before:], "hs_split_bf16x3") == 4, called  # both weight splits were made again
    assert torch.equal(y, _f32(y2)), "y after the write"
    assert torch.equal(x.grad, _f32(dx2)), "dx after the write"


# ----------------------------------------------------------------------------- B. _weight_split follows the weights
B_SHAPE = (328, 320)
B_ROWS = 33


def _product(x, w, b=None):
    from heal_swin_amd import ops
    with torch.no_grad():
        return ops.linear(x, w, b)


def test_raw_pointer_update_is_seen_once_the_epoch_has_moved():
    """torch._foreach_add_ on [p.data] leaves `_version` alone (as fused optimizers do): the cached split is served until
    RT.weight_epoch moves -- that is the cache's contract -- and the new product afterwards."""
    from heal_swin_amd import ops
    c = _case(B_ROWS, *B_SHAPE)
    _assert_bf16x3(c)
    (_, w2p), (_, w2) = _weights(*B_SHAPE, 2, 11)
    w = torch.nn.Parameter(c.w.clone())
    assert torch.equal(_product(c.x, w), c.y)
    _raw_write(w, w2)
    assert torch.equal(_product(c.x, w), c.y), "same epoch, same version: the cached operand"
    ops.RT.weight_epoch += 1
    assert torch.equal(_product(c.x, w), _f32(_x3(c.xp, w2p))), "new epoch: the weights as they are now"


def test_note_forward_opens_an_epoch_for_grad_and_the_first_no_grad_forward(monkeypatch):
    """note_forward's rule as a sequence: a grad-enabled forward opens an epoch (an optimizer step follows), the first no-grad forward
    after it one more (it follows that step), later no-grad forwards none (evaluation loops re-use the operands)."""
    from heal_swin_amd import ops
    c = _case(B_ROWS, *B_SHAPE)
    _assert_bf16x3(c)
    parts, values = _weights(*B_SHAPE, 4, 13)
    refs = [_f32(_x3(c.xp, p)) for p in parts]
    monkeypatch.setattr(ops.RT, "_epoch_dirty", False)  # (restored at the end)
    w = torch.nn.Parameter(values[0].clone())
    assert torch.equal(_product(c.x, w), refs[0])
    epoch = ops.RT.weight_epoch
    _raw_write(w, values[1])
    ops.note_forward(True)
    assert ops.RT.weight_epoch == epoch + 1 and torch.equal(_product(c.x, w), refs[1]), "grad-enabled forward"
    _raw_write(w, values[2])
    ops.note_forward(False)
    assert ops.RT.weight_epoch == epoch + 2 and torch.equal(_product(c.x, w), refs[2]), "first no-grad forward after it"
    _raw_write(w, values[3])
    ops.note_forward(False)
    assert ops.RT.weight_epoch == epoch + 2 and torch.equal(_product(c.x, w), refs[2]), "second no-grad forward: the cached operand"
    ops.RT.weight_epoch += 1
    assert torch.equal(_product(c.x, w), refs[3])


def test_flat_adam_step_moves_the_epoch():
    """FlatAdam.step() updates through raw pointers.  With zero gradients, lr = 0.5 and decoupled weight decay 1 the step is
    p *= 0.5 exactly: the operands stay in the class (every part halves), the product after the step must be half the one before."""
    from heal_swin_amd import ops
    from heal_swin_amd.optim import FlatAdam
    from heal_swin_amd.parallel import GradBucketAllReduce
    c = _case(B_ROWS, *B_SHAPE)
    _assert_bf16x3(c)
    w, b = torch.nn.Parameter(c.w.clone()), torch.nn.Parameter(c.b.clone())
    sink = GradBucketAllReduce([w, b])
    try:
        opt = FlatAdam([w, b], sink, lr=0.5, weight_decay=1.0, decoupled_weight_decay=True)
        assert torch.equal(_product(c.x, w, b), c.y_b)
        epoch, version = ops.RT.weight_epoch, w._version
        sink.zero_grad()
        opt.step()
        assert w._version == version and torch.equal(w.data, c.w * 0.5) and torch.equal(b.data, c.b * 0.5)
        assert ops.RT.weight_epoch > epoch
        assert torch.equal(_product(c.x, w, b), _f32((c.y_b * 0.5).double())), "the product of the stepped weights"
    finally:
        sink.remove()


def test_weight_split_cache_stays_bounded(monkeypatch):
    """More weights than _WSPLIT_CAPACITY: the oldest entries go, the cache stays bounded, and an evicted weight is split again."""
    G = _G()
    c = _case(B_ROWS, *B_SHAPE)
    _assert_bf16x3(c)
    w = torch.nn.Parameter(c.w.clone())
    assert torch.equal(_product(c.x, w), c.y)
    key = next(k for k in G._WSPLIT if k[0] == w.untyped_storage().data_ptr())
    small = torch.ones((G._WSPLIT_CAPACITY + 8, 8, 8), device=DEV)
    for i in range(small.shape[0]):
        G._weight_split(small[i], False)
        assert len(G._WSPLIT) <= G._WSPLIT_CAPACITY
    assert key not in G._WSPLIT
    called = spy_on(monkeypatch, CENSUS, [G])
    assert torch.equal(_product(c.x.clone(), w), c.y) and _count(called, "hs_split_bf16x3") == 2 and key in G._WSPLIT  # x and the weight
    for k in [k for k, v in G._WSPLIT.items() if v[2].untyped_storage().data_ptr() == small.untyped_storage().data_ptr()]:
        del G._WSPLIT[k]


# ----------------------------------------------------------------------------- C. the fp32 step under graph replay
def _build32(seed=0):
    """The model of tests/test_gpu_graphs.py at embed_dim 128 in fp32: stage 1 (C = 256) has qkv, fc1 and fc2 on the bf16x3 path."""
    from heal_swin_amd.data_spec import DataSpec
    from heal_swin_amd.models_torch.swin_hp_transformer import SwinHPTransformerConfig, SwinHPTransformerSys

    cfg = dict(patch_size=4, window_size=64, shift_size=32, shift_strategy="nest_roll", rel_pos_bias="flat", embed_dim=128,
               depths=[2, 2], num_heads=[4, 8], mlp_ratio=4.0, qkv_bias=True, qk_scale=None, use_cos_attn=False, drop_rate=0.0,
               attn_drop_rate=0.0, drop_path_rate=0.0, use_v2_norm_placement=False, ape=False)
    spec = dict(dim_in=8 * 16 * 16, f_in=3, f_out=12, base_pix=8, class_names=[])
    torch.manual_seed(seed)
    model = SwinHPTransformerSys(SwinHPTransformerConfig(**cfg), DataSpec(**spec)).cuda().train()
    model.compute_dtype = torch.float32
    return model, spec


def _batches(spec, n, batch=2):
    g = torch.Generator(device="cuda").manual_seed(7)
    return [(torch.randint(0, 256, (batch, 3, spec["dim_in"]), generator=g, device="cuda", dtype=torch.uint8),
             torch.randint(0, spec["f_out"], (batch, spec["dim_in"]), generator=g, device="cuda", dtype=torch.uint8)) for _ in range(n)]


def _optimizer(kind, model, sink, lr):
    from heal_swin_amd.optim import FlatAdam
    from heal_swin_amd.parallel import GradBucketAllReduce
    dp = GradBucketAllReduce(model.parameters()) if sink else None
    if kind == "flat":
        return dp, FlatAdam(model.parameters(), dp, lr=lr, model=model)
    return dp, torch.optim.Adam(model.parameters(), lr=lr, fused=True, capturable=True)


def _eager_step(model, opt, dp, x, y):
    from heal_swin_amd.losses import seg_loss
    if dp is not None:
        dp.zero_grad()
    else:
        opt.zero_grad(set_to_none=False)
    loss = seg_loss(model(x.float()), y)
    loss.backward()
    if dp is not None:
        dp.finish()
    opt.step()
    return loss.detach()


def _assert_stage1_on_bf16x3(called):
    """Census of one eager training step: in each stage-1 block (at least the encoder's two) qkv, fc1 and fc2 run three
    hs_linear_wgrad_ld each -- nothing else calls that entry point -- and the Mlp writes gelu(h) and dh as splits (hs_gelu_split3)."""
    assert _count(called, "hs_linear_wgrad_ld") >= 2 * 3 * 3 and _count(called, "hs_linear_wgrad_ld") % 3 == 0, called
    assert _count(called, "hs_gelu_split3") >= 2 * 2, called
    assert _count(called, "hs_split_bf16x3") > 0, called


@pytest.mark.parametrize("kind,sink", [("adam", False), ("adam", True), ("flat", True)])
def test_graphed_fp32_step_equals_eager_step(kind, sink, monkeypatch):
    """The fp32 twin of test_gpu_graphs.py::test_graphed_step_equals_eager_step: losses and final parameters of four replayed steps
    equal the eager run's (the bf16x3 products go through the library GEMM; its algorithm choice is the same in both runs)."""
    from heal_swin_amd import ops
    from heal_swin_amd.graphs import GraphedTrainStep
    from heal_swin_amd.losses import seg_loss

    losses, finals = {}, {}
    for mode in ("eager", "graph"):
        model, spec = _build32()
        data = _batches(spec, 5)
        dp, opt = _optimizer(kind, model, sink, 1e-3)
        try:
            if mode == "graph":
                step = GraphedTrainStep(model, seg_loss, opt, data[0][0], data[0][1], warmup=2, pre_forward=lambda x: x.float(), grad_sink=dp)
                out = [float(step(x, y)) for x, y in data[1:]]
            else:
                with monkeypatch.context() as mp:
                    called = spy_on(mp, CENSUS, [ops.gemm, ops.mlp_branch])
                    _eager_step(model, opt, dp, *data[0])
                _assert_stage1_on_bf16x3(called)
                _eager_step(model, opt, dp, *data[0])  # the second warm-up step
                out = [float(_eager_step(model, opt, dp, x, y)) for x, y in data[1:]]
            losses[mode] = out
            finals[mode] = {k: v.detach().clone() for k, v in model.named_parameters()}
        finally:
            if dp is not None:
                dp.remove()
    assert losses["eager"] == losses["graph"], (losses["eager"], losses["graph"])
    for k, v in finals["eager"].items():
        assert torch.equal(v, finals["graph"][k]), k


@pytest.mark.parametrize("kind,sink", [("adam", False), ("flat", True)])
def test_fp32_evaluation_between_replays_sees_the_current_weights(kind, sink):
    """replay -> eval, four rounds, in fp32: the eager no-grad logits after each replay must equal, bit for bit, those of a FRESH model
    built from state_dict() copies of the graphed model's current parameters (no cache history, no second training run).  A replay
    runs no Python: neither `_version` of a weight nor -- by itself -- RT.weight_epoch moves, so the bf16x3 weight splits made for
    the previous evaluation would be served again; GraphedTrainStep moves the epoch after every replay.  (Without that the second
    evaluation failed here, with both optimizers: logits off by 5.6e-3 at the largest.)"""
    from heal_swin_amd.graphs import GraphedTrainStep
    from heal_swin_amd.losses import seg_loss

    model, spec = _build32()
    data = _batches(spec, 5)
    dp, opt = _optimizer(kind, model, sink, 1e-2)
    xe = data[0][0].float()

    def evaluate(m):
        m.eval()
        with torch.no_grad():
            y = m(xe).float().clone()
        m.train()
        return y

    try:
        step = GraphedTrainStep(model, seg_loss, opt, data[0][0], data[0][1], warmup=2, pre_forward=lambda x: x.float(), grad_sink=dp)
        weight = model.layers[1].blocks[0].mlp.fc1.weight
        assert weight.shape == (1024, 256) and weight.dtype == torch.float32
        logits = []
        for i, (x, y) in enumerate(data[1:]):
            version, before = weight._version, weight.detach().clone()
            step(x, y)
            assert weight._version == version and not torch.equal(weight.detach(), before), f"replay {i}"
            got = evaluate(model)
            fresh, _ = _build32(seed=1)
            fresh.load_state_dict({k: v.detach().clone() for k, v in model.state_dict().items()})
            want = evaluate(fresh)
            assert torch.equal(got, want), f"eval after replay {i}: max diff {float((got - want).abs().max())}"
            logits.append(got)
        for i in range(1, len(logits)):
            assert not torch.equal(logits[i - 1], logits[i]), f"the logits did not move between rounds {i - 1} and {i}"
    finally:
        if dp is not None:
            dp.remove()
