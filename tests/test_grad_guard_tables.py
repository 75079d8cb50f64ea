"""The host side of the gradient guard (optim.GradGuard, csrc/grad_guard.hip): the item / parameter tables the kernels are driven by,
FlatAdam's new arguments and the bindings of the new entry points.  No GPU needed."""
import inspect

import pytest

SHAPES = [(64, 32), (64,), (7, 5, 3), (1,), (129, 33), (1000,), (3, 1, 1), ("PIECE+1",), ("2*PIECE+8",)]


@pytest.fixture(scope="module")
def optim():
    import __graft_entry__ as g
    g.build()
    from heal_swin_amd import optim
    return optim


def _numel(shape, piece):
    n = 1
    for d in shape:
        n *= {"PIECE+1": piece + 1, "2*PIECE+8": 2 * piece + 8}.get(d, d)
    return n


def _layout(piece, bucket_elems=4096, slot=8):
    """The slots parallel.GradBucketAllReduce gives these shapes: reversed order, each rounded up to a multiple of `slot` elements, a new
    bucket when the next slot would not fit."""
    layout, cur, off = [], [], 0
    for i in reversed(range(len(SHAPES))):
        n = _numel(SHAPES[i], piece)
        size = -(-n // slot) * slot
        if cur and off + size > bucket_elems:
            layout.append(cur)
            cur, off = [], 0
        cur.append((i, off, n))
        off += size
    layout.append(cur)
    return layout


def test_item_table_covers_every_element_once(optim):
    piece = optim.grad_piece()
    assert piece % 4 == 0 and 1024 <= piece <= 16384, "a few thousand elements, whole 16-byte loads"
    layout = _layout(piece)
    assert len(layout) > 1
    items, params = optim.guard_tables(layout, piece)
    assert len(items) == len(layout) and len(params) == len(SHAPES)
    first_of_bucket, n = [], 0
    for it in items:
        first_of_bucket.append(n)
        n += len(it)
    seen_params = set()
    for b, bucket in enumerate(layout):
        covered = {}
        for k, (start, length) in enumerate(items[b]):
            assert 0 < length <= piece and start % 4 == 0, (b, k, start, length)
            owners = [i for i, off, numel in bucket if off <= start and start + length <= off + numel]
            assert len(owners) == 1, f"item {(start, length)} of bucket {b} lies in no single parameter"
            first, count = params[owners[0]]
            assert first <= first_of_bucket[b] + k < first + count, "the items of a parameter are consecutive, where its table entry says"
            for e in range(start, start + length):
                assert e not in covered, "an element in two items"
                covered[e] = owners[0]
        for i, off, numel in bucket:
            assert all(covered.get(e) == i for e in range(off, off + numel)), f"parameter {i}: an element in no item"
            assert params[i][1] == -(-numel // piece)
            seen_params.add(i)
        assert len(covered) == sum(numel for _, _, numel in bucket), "the gaps between slots belong to no item"
    assert seen_params == set(range(len(SHAPES)))
    assert sorted(f for f, _ in params) == sorted(set(f for f, _ in params)) and sum(c for _, c in params) == n
    # exact and off-by-one multiples of the piece
    assert params[7][1] == 2 and params[8][1] == 3
    assert optim.guard_tables([[(0, 0, piece)]], piece) == ([[(0, piece)]], [(0, 1)])


def test_item_table_refuses_what_the_kernels_cannot_load(optim):
    with pytest.raises(ValueError):
        optim.guard_tables([[(0, 2, 10)]], 4096)  # a slot off a 16-byte boundary
    with pytest.raises(ValueError):
        optim.guard_tables([[(0, 0, 10), (2, 16, 3)]], 4096)  # parameter 1 missing


def test_flat_adam_signature_carries_the_guard_arguments(optim):
    sig = inspect.signature(optim.FlatAdam.__init__).parameters
    for name, default in (("max_grad_norm", None), ("clip_value", None), ("norm_type", 2.0), ("skip_nonfinite", False), ("track_grad_norm", False)):
        assert name in sig and sig[name].default == default, name
    for prop in ("grad_norm", "param_grad_norms", "skipped_steps"):
        assert isinstance(getattr(optim.FlatAdam, prop), property)
    from heal_swin_amd import parallel
    assert list(inspect.signature(parallel.clip_grad_norm_).parameters) == ["sink", "max_norm", "norm_type"]
    assert "synchronis" in optim.GradGuard.named_norms.__doc__.lower()


def test_new_entry_points_are_bound(optim):
    from heal_swin_amd import _lib
    for name in ("hs_grad_stats", "hs_grad_guard_finalize", "hs_adam_step_guarded", "hs_adam_advance_guarded", "hs_grad_scale", "hs_grad_guard_piece"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib, name), name
