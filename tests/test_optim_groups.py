"""The host side of FlatAdam's parameter groups (optim.group_tables, optim.weight_decay_groups, csrc/adam.hip's grouped entry points):
the ownership tables the kernel is driven by, the weight-decay split from the models' own declarations, the bindings and the
constructor's refusals.  No GPU needed."""
import pytest

from test_grad_guard_tables import _layout

BLOCK = 1024


@pytest.fixture(scope="module")
def optim():
    import __graft_entry__ as g
    g.build()
    from heal_swin_amd import optim
    return optim


def _alternating(layout):
    """Two groups, alternating along every bucket (in slot order: neighbours differ)."""
    groups = ([], [])
    for bucket in layout:
        for k, (index, _, _) in enumerate(sorted(bucket, key=lambda e: e[1])):
            groups[k % 2].append(index)
    return groups


def _run_of(runs, e):
    return max(r for r, (start, _) in enumerate(runs) if start <= e)


def test_group_tables_own_every_element_and_point_at_the_first_run(optim):
    layout = _layout(optim.grad_piece())
    assert len(layout) > 1
    groups = _alternating(layout)
    group_of = {i: k for k, members in enumerate(groups) for i in members}
    runs, block_first = optim.group_tables(layout, groups, block=BLOCK)
    assert len(runs) == len(block_first) == len(layout)
    one_run_blocks = many_run_blocks = gaps = 0
    for bucket, rs, first in zip(layout, runs, block_first):
        slots = sorted(bucket, key=lambda e: e[1])
        length = -(-(slots[-1][1] + slots[-1][2]) // 8) * 8
        assert rs[0][0] == 0 and all(s % 8 == 0 for s, _ in rs) and [s for s, _ in rs] == sorted(set(s for s, _ in rs))
        assert all(a[1] != b[1] for a, b in zip(rs, rs[1:])), "runs are maximal: neighbours differ in group"
        owner = [rs[_run_of(rs, e)][1] for e in range(length)]
        for k, (index, off, numel) in enumerate(slots):
            assert set(owner[off:off + numel]) == {group_of[index]}, f"parameter {index}: an element owned by another group"
            end = slots[k + 1][1] if k + 1 < len(slots) else length
            if end > off + numel:  # the gap behind a slot (and the bucket's tail) goes with the run in front of it
                gaps += 1
                assert set(owner[off + numel:end]) == {group_of[index]}
        assert len(first) == -(-length // BLOCK)
        for b, r in enumerate(first):
            assert r == _run_of(rs, b * BLOCK), "the block table points at the run that holds the block's first element"
            inside = len({_run_of(rs, e) for e in range(b * BLOCK, min((b + 1) * BLOCK, length), 8)})
            one_run_blocks += inside == 1
            many_run_blocks += inside > 2
    assert gaps > 0 and one_run_blocks > 0 and many_run_blocks > 0, (gaps, one_run_blocks, many_run_blocks)
    # consecutive slots of one group are one run; an explicit bucket length adds blocks, not runs
    assert optim.group_tables([[(0, 0, 10), (1, 16, 3), (2, 24, 2000)]], [[0, 1], [2]]) == ([[(0, 0), (24, 1)]], [[0, 1]])
    assert optim.group_tables([[(0, 0, 10), (1, 16, 3)]], [[0], [1]], lengths=[2056]) == ([[(0, 0), (16, 1)]], [[0, 1, 1]])
    assert optim.group_tables([[(0, 0, 10)], [(1, 0, 3)]], [[1, 0]]) == ([[(0, 0)], [(0, 0)]], [[0], [0]])


def test_group_tables_refuse_what_the_kernel_cannot_load(optim):
    with pytest.raises(ValueError):
        optim.group_tables([[(0, 0, 10), (1, 12, 3)]], [[0], [1]])  # a slot off an 8-element boundary
    with pytest.raises(ValueError):
        optim.group_tables([[(0, 0, 10), (1, 16, 3)]], [[0]])  # parameter 1 in no group
    with pytest.raises(ValueError):
        optim.group_tables([[(0, 0, 10), (1, 16, 3)]], [[0, 1], [1]])  # parameter 1 in two
    most = optim.adam_max_groups()
    layout = [[(i, 8 * i, 3) for i in range(most + 1)]]
    with pytest.raises(ValueError):
        optim.group_tables(layout, [[i] for i in range(most + 1)])  # more groups than one launch takes
    runs, _ = optim.group_tables([layout[0][:most]], [[i] for i in range(most)])
    assert len(runs[0]) == most


def _tiny_models():
    from heal_swin_amd.data_spec import DataSpec
    from heal_swin_amd.models_torch.swin_hp_transformer import SwinHPTransformerConfig, SwinHPTransformerSys
    from heal_swin_amd.models_torch.swin_transformer import SwinTransformerConfig, SwinTransformerSys
    from _golden import model_cfg_spec
    cfg, spec = model_cfg_spec("bp12_roll_v2cos")  # (tests/test_cabi.py's tiny models: position-bias tables on, cosine attention)
    assert cfg["rel_pos_bias"] == "flat" and cfg["use_cos_attn"]
    yield "hp", SwinHPTransformerSys(SwinHPTransformerConfig(**dict(cfg, ape=True)), DataSpec(**spec))
    flat_spec = DataSpec(dim_in=(64, 64), f_in=3, f_out=4, base_pix=None, class_names=[])
    yield "flat", SwinTransformerSys(SwinTransformerConfig(patch_size=2, window_size=4, embed_dim=16, depths=[2, 2], num_heads=[1, 2],
                                                           use_cos_attn=True, ape=True, drop_path_rate=0.0), flat_spec)


def test_weight_decay_groups_follow_the_models_declarations(optim):
    import torch
    seen = set()
    for kind, model in _tiny_models():
        names = {id(p): n for n, p in model.named_parameters()}
        trainable = [p for p in model.parameters() if p.requires_grad]
        decay, no_decay = optim.weight_decay_groups(model, 0.05, lr=2e-4)
        assert decay["weight_decay"] == 0.05 and no_decay["weight_decay"] == 0.0 and decay["lr"] == no_decay["lr"] == 2e-4
        ids = [id(p) for p in decay["params"]] + [id(p) for p in no_decay["params"]]
        assert sorted(ids) == sorted(map(id, trainable)), f"{kind}: every trainable parameter in exactly one group"
        nd = {names[id(p)] for p in no_decay["params"]}
        for n, p in model.named_parameters():
            if not p.requires_grad:
                continue
            if n.endswith((".bias", "logit_scale", "relative_position_bias_table", "absolute_pos_embed")) or "norm" in n.split(".")[-2]:
                assert n in nd, f"{kind}: {n} must not decay"
                seen.add(n.split(".")[-1] if "norm" not in n else "norm")
        for mn, mod in model.named_modules():
            if isinstance(mod, (torch.nn.Linear, torch.nn.Conv2d)) or type(mod).__name__ == "HSLinear":
                assert mn + ".weight" not in nd, f"{kind}: the weight of {mn} decays"
        assert len(decay["params"]) > 0
        # without the 1-d rule: only what no_weight_decay() / no_weight_decay_keywords() name
        decay2, no_decay2 = optim.weight_decay_groups(model, 0.05, no_decay_1d=False)
        named = {n for n, p in model.named_parameters() if p.requires_grad and
                 (n.endswith("absolute_pos_embed") or "relative_position_bias_table" in n)}
        assert {names[id(p)] for p in no_decay2["params"]} == named and named
        assert len(decay2["params"]) + len(no_decay2["params"]) == len(trainable)
    assert {"bias", "logit_scale", "relative_position_bias_table", "norm"} <= seen, seen


def test_grouped_entry_points_are_bound(optim):
    from heal_swin_amd import _lib
    for name in ("hs_adam_step_groups", "hs_adam_step_groups_guarded", "hs_adam_max_groups"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib, name), name
    assert optim.adam_max_groups() == _lib.lib.hs_adam_max_groups() >= 32
    import ctypes
    assert ctypes.sizeof(_lib.AdamGroup) == 32, "hs_adam_group: a pointer, five floats, one int32"
    # refused on the host before anything touches a device: no groups, too many
    rec = _lib.adam_groups([(1e-3, 0.9, 0.999, 1e-8, 0.0, False)] * (optim.adam_max_groups() + 1))
    buf = ctypes.create_string_buffer(4096 + 16)
    P = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    for n_groups in (0, optim.adam_max_groups() + 1):
        st = _lib.lib.hs_adam_step_groups(P, P, P, P, None, 1024, rec, n_groups, P, 1, P, 1, 1024, P, None)
        assert st == 1 and "group count" in _lib.lib.hs_last_error().decode(), n_groups


def test_flat_adam_constructor_refusals_that_need_no_device(optim):
    import torch

    class Sink:  # (the constructor looks at the sink's parameter list before anything else of it)
        def __init__(self, params):
            self.params = list(params)
    a, b, frozen = (torch.nn.Parameter(torch.zeros(4)) for _ in range(3))
    frozen.requires_grad_(False)
    with pytest.raises(ValueError, match="holds no parameter"):
        optim.FlatAdam([dict(params=[a, b]), dict(params=[frozen])], Sink([a, b]))
    with pytest.raises(ValueError, match="more than one parameter group"):
        optim.FlatAdam([dict(params=[a, b]), dict(params=[b])], Sink([a, b]))
    with pytest.raises(ValueError, match="same parameters"):
        optim.FlatAdam([dict(params=[a]), dict(params=[b])], Sink([a]))
    many = [torch.nn.Parameter(torch.zeros(1)) for _ in range(optim.adam_max_groups() + 1)]
    with pytest.raises(ValueError, match="at most"):
        optim.FlatAdam([dict(params=[p]) for p in many], Sink(many))
    for bad in (dict(betas=(0.9, 1.0)), dict(eps=-1.0), dict(weight_decay=-0.1)):
        with pytest.raises(ValueError, match="hyper-parameters"):
            optim.FlatAdam([dict(params=[a]), dict(params=[b], **bad)], Sink([a, b]))
    with pytest.raises(ValueError, match="not both"):
        optim.FlatAdam([dict(params=[a])], Sink([a]), max_grad_norm=1.0, clip_value=1.0)
    with pytest.raises(RuntimeError, match="no CPU path"):  # and still no CPU path, with groups as without
        optim.FlatAdam([dict(params=[a]), dict(params=[b], lr=1e-4)], Sink([a, b]))
