"""FlatAdam: torch.optim.Adam / AdamW (what the reference's trainer builds, heal_swin/training/optimizer.py:57-66) on flat buffers.

    dp = GradBucketAllReduce(model.parameters())            # gradients: a few flat fp32 buckets (parallel.py)
    opt = FlatAdam(model.parameters(), dp, lr=1e-3, model=model)
    ...
    dp.zero_grad(); loss.backward(); dp.finish(); opt.step()

Parameters and both moments are laid out exactly like the gradient buckets (every `p.data` becomes a view into a flat fp32
buffer; values are preserved), so a step is ONE `hs_adam_step` launch per bucket (csrc/adam.hip) -- and that launch also writes
the bf16 copy of the updated parameters that the model's next forward reads (`ops.ParamCastCache`), which otherwise costs a
second pass over all parameters per training step.  Same arithmetic as torch.optim.Adam (amsgrad = False, maximize = False;
`decoupled_weight_decay=True` = AdamW); the step counter lives on the device, so the whole training step stays capturable in
one HIP graph (`graphs.GraphedTrainStep`, `bench.py --graph`).

It is a torch.optim.Optimizer: learning-rate schedulers act on `param_groups[i]["lr"]` (read on the host at every `step()`; under
graph replay pass `lr` as a 0-dim CUDA tensor and update it in place), `state_dict()` / `load_state_dict()` carry `exp_avg`,
`exp_avg_sq` and `step` per parameter in torch.optim.Adam's layout.  GPU only -- there is no CPU path.

Parameter groups: `params` may be a list of dicts with their own `lr` (float or device tensor, mixed freely), `betas`, `eps`,
`weight_decay`, `decoupled_weight_decay`; `weight_decay_groups(model, wd)` makes the usual Swin split (no decay on biases, LayerNorm
parameters, position tables, `logit_scale`) from the model's own `no_weight_decay()` / `no_weight_decay_keywords()`.  A step stays
one launch per bucket (`hs_adam_step_groups`): the groups' hyper-parameters travel as kernel arguments, and a static table per
bucket (`group_tables`) tells the kernel which group owns an element.  Groups are fixed at construction (up to `adam_max_groups()`).

Guard rails (the reference trainer's gradient_clip_val / gradient_clip_algorithm, track_grad_norm, terminate_on_nan:
training/train_config.py:65-66,76,104): `max_grad_norm=` / `clip_value=`, `track_grad_norm=True`, `skip_nonfinite=True`.  With any of
them `step()` first measures the buckets (`GradGuard`: one read-only pass, csrc/grad_guard.hip) and then runs the guarded Adam
launches, which take the clip coefficient and the finite flag from device memory -- no host read, the step stays capturable.

Weight averaging (the reference trainer's stochastic_weight_avg, training/train_config.py:112, and its every-step form, EMA):
`FlatWeightAverage(optimizer, "swa" | "ema")` keeps the average in one more flat buffer per bucket, updates it with one
`hs_weight_avg_update` launch per bucket (csrc/weight_avg.hip) and swaps it into the model for validation, bf16 copies included.
"""
import contextlib
import math

import torch

from . import _lib, ops
from ._lib import check, lib, ptr, stream_ptr


def grad_piece():
    """PIECE: the most elements one item of the guard's table covers (a compile-time constant of csrc/grad_guard.hip)."""
    return int(lib.hs_grad_guard_piece())


def guard_tables(layout, piece):
    """The tables `hs_grad_stats` / `hs_grad_guard_finalize` are driven by (pure host code).
    layout: per bucket, a list of (parameter index, element offset in the bucket, numel); offsets are multiples of 4.
    Returns (items, params): items[b] = [(start, len), ...] for bucket b -- every parameter cut into consecutive slices of at most
    `piece` elements, no slice crossing a parameter boundary -- and params[i] = (first item, item count) of parameter i, items
    numbered through all buckets in order."""
    n_params = sum(len(bucket) for bucket in layout)
    items, params, first = [], [None] * n_params, 0
    for bucket in layout:
        cur = []
        for index, off, numel in sorted(bucket, key=lambda e: e[1]):
            if off % 4 or piece % 4:
                raise ValueError("a parameter's slot and the piece size must be multiples of 4 elements (16-byte loads)")
            if not 0 <= index < n_params or params[index] is not None:
                raise ValueError("parameter indices must be 0 ... n - 1, each once")
            count = -(-numel // piece)
            cur += [(off + k * piece, min(piece, numel - k * piece)) for k in range(count)]
            params[index] = (first, count)
            first += count
        items.append(cur)
    return items, params


def adam_max_groups():
    """HS_ADAM_MAX_GROUPS: the most parameter groups one `hs_adam_step_groups` launch takes (a compile-time constant of csrc/adam.hip)."""
    return int(lib.hs_adam_max_groups())


def group_tables(layout, groups, block=1024, lengths=None):
    """The tables `hs_adam_step_groups` finds an element's parameter group by (pure host code).
    layout: as for `guard_tables` -- per bucket, a list of (parameter index, element offset in the bucket, numel) -- with offsets that
    are multiples of 8 (the sink's slot rule: a float4 never straddles two parameters); groups: per group, the indices of its parameters;
    lengths: the element count of every bucket (default: up to the end of its last slot, rounded up to 8).
    Returns (runs, block_first): runs[b] = [(first element, group), ...] for bucket b -- consecutive slots of one group merged into
    one run, the gap behind a slot belonging to the run in front of it, the first run starting at 0 -- and block_first[b][k] = the run that
    holds element k * block of bucket b.  ValueError for what the kernel cannot load: a slot off an 8-element boundary, a parameter in no
    group or in two, more groups than `adam_max_groups()`."""
    max_groups = adam_max_groups()
    groups = [list(members) for members in groups]
    if not 1 <= len(groups) <= max_groups:
        raise ValueError(f"{len(groups)} parameter groups: one launch takes 1 ... {max_groups}")
    n_params = sum(len(bucket) for bucket in layout)
    group_of = {}
    for k, members in enumerate(groups):
        for index in members:
            if index in group_of:
                raise ValueError(f"parameter {index} is in more than one group")
            group_of[index] = k
    if sorted(group_of) != list(range(n_params)):
        raise ValueError("every parameter 0 ... n - 1 of the layout must be in exactly one group")
    runs, block_first = [], []
    for b, bucket in enumerate(layout):
        cur, end = [], 0
        for index, off, numel in sorted(bucket, key=lambda e: e[1]):
            if off % 8 or off < end:
                raise ValueError("a parameter's slot must start on a multiple of 8 elements, behind the slot in front of it")
            if not cur or cur[-1][1] != group_of[index]:
                cur.append((off if cur else 0, group_of[index]))
            end = off + numel
        length = -(-end // 8) * 8 if lengths is None else int(lengths[b])
        if not cur or length < end:
            raise ValueError("a bucket holds at least one parameter and all of its last one")
        starts = [s for s, _ in cur]
        first, r = [], 0
        for e in range(0, length, block):
            while r + 1 < len(starts) and starts[r + 1] <= e:
                r += 1
            first.append(r)
        runs.append(cur)
        block_first.append(first)
    return runs, block_first


def weight_decay_groups(model, weight_decay, no_decay_1d=True, **group_options):
    """[decay group, no-decay group] for FlatAdam (or torch.optim.AdamW) from the model's own declarations, Swin's `set_weight_decay` rule:
    without decay are the parameters whose name ends in an entry of `model.no_weight_decay()` (absolute_pos_embed) or contains an entry
    of `model.no_weight_decay_keywords()` (the relative-position bias tables) and, with `no_decay_1d`, every parameter with ndim <= 1 --
    biases, LayerNorm weights -- and the cosine attention's per-head `logit_scale`, a vector stored as [heads, 1, 1].  Parameters that
    do not require a gradient are in neither.  group_options (lr=, betas=, ...) go into both groups.  Pure host code."""
    skip = set(getattr(model, "no_weight_decay", set)())
    keywords = set(getattr(model, "no_weight_decay_keywords", set)())
    decay, no_decay = [], []
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        named = any(name.endswith(s) for s in skip) or any(k in name for k in keywords)
        one_d = no_decay_1d and (p.ndim <= 1 or name.endswith("logit_scale"))
        (no_decay if named or one_d else decay).append(p)
    return [dict(group_options, params=decay, weight_decay=float(weight_decay)), dict(group_options, params=no_decay, weight_decay=0.0)]


def _norm_kind(norm_type):
    norm_type = float(norm_type)
    if norm_type not in (2.0, math.inf):
        raise ValueError("the gradient guard measures the 2-norm or the inf-norm")
    return norm_type


class GradGuard:
    """Norms of the gradients in a parallel.GradBucketAllReduce's buckets, and the device record a guarded step acts on.

    `measure()` is one `hs_grad_stats` launch per bucket plus `hs_grad_guard_finalize`, all on the current stream and capturable;
    afterwards `total_norm` (0-dim fp32), `param_norms` ([n_params] fp32, in `sink.params` order), `clip_coef` and `finite` hold the
    result ON THE DEVICE.  Sums are fp64 in an order fixed by the tables built here once: the same buckets give the same bits,
    on every rank of a data-parallel run after the exchange."""

    def __init__(self, sink, norm_type=2.0):
        self.norm_type = _norm_kind(norm_type)
        self.sink = sink
        if not sink.buckets or not sink.buckets[0].is_cuda:
            raise RuntimeError("GradGuard runs on the gradient buckets of an MI355X (HIP) device; there is no CPU path")
        dev = sink.buckets[0].device
        layout = [[] for _ in sink.buckets]
        for i, p in enumerate(sink.params):
            b = sink._where[p]
            layout[b].append((i, sink._views[p].storage_offset() - sink.buckets[b].storage_offset(), p.numel()))
        items, params = guard_tables(layout, grad_piece())
        self._items = [torch.tensor(it, dtype=torch.int64, device=dev).reshape(len(it), 2) for it in items]
        self._first = [sum(len(it) for it in items[:b]) for b in range(len(items))]
        self.n_items = sum(len(it) for it in items)
        self._params = torch.tensor(params, dtype=torch.int32, device=dev).reshape(len(params), 2)
        self.partials = torch.zeros(max(self.n_items, 1), 2, dtype=torch.float64, device=dev)  # per item: sum of squares, max |g|
        self._work = torch.zeros(len(params), 2, dtype=torch.float64, device=dev)
        self.param_norms = torch.zeros(len(params), dtype=torch.float32, device=dev)
        self.record = torch.zeros(4, dtype=torch.float32, device=dev)  # hs_grad_guard: total_norm, clip_coef, finite (int32), -
        self.record[1] = 1.0
        self.total_norm, self.clip_coef = self.record[0], self.record[1]
        self.finite = self.record.view(torch.int32)[2]

    def measure(self, max_norm=None):
        """Launch the measurement of the buckets as they are now; max_norm: clip_coef = min(1, max_norm / (total_norm + 1e-6)),
        None: 1.  Returns `total_norm` (a device tensor; nothing is read on the host)."""
        s = stream_ptr(self.record.device)
        for G, items, first in zip(self.sink.buckets, self._items, self._first):
            if len(items):
                check(lib.hs_grad_stats(ptr(G), G.numel(), ptr(items), len(items), ptr(self.partials[first:]), s), "hs_grad_stats")
        check(lib.hs_grad_guard_finalize(ptr(self.partials), self.n_items, ptr(self._params), self._params.shape[0],
                                         int(self.norm_type == math.inf), -1.0 if max_norm is None else float(max_norm),
                                         ptr(self.param_norms), ptr(self._work), ptr(self.record), s), "hs_grad_guard_finalize")
        return self.total_norm

    def scale_(self, clip_value=None):
        """Clamp the buckets to +-clip_value (if given) and scale them by the measured `clip_coef`, in place (`hs_grad_scale`)."""
        s = stream_ptr(self.record.device)
        for G in self.sink.buckets:
            check(lib.hs_grad_scale(ptr(G), G.numel(), 0.0 if clip_value is None else float(clip_value), ptr(self.record), s), "hs_grad_scale")

    def named_norms(self, model):
        """{"grad_<p>_norm_<parameter name>": float, ..., "grad_<p>_norm_total": float} of the last `measure()`, <p> the norm type
        (2.0 or inf): the keys Lightning's track_grad_norm logs.  SYNCHRONISES: the norms are copied to the host."""
        names = {id(p): n for n, p in model.named_parameters()}
        values = self.param_norms.tolist()
        out = {f"grad_{self.norm_type}_norm_{names[id(p)]}": v for p, v in zip(self.sink.params, values) if id(p) in names}
        out[f"grad_{self.norm_type}_norm_total"] = float(self.total_norm)
        return out


class FlatAdam(torch.optim.Optimizer):
    def __init__(self, params, grad_sink, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled_weight_decay=False,
                 model=None, lowp_dtype=torch.bfloat16, max_grad_norm=None, clip_value=None, norm_type=2.0, skip_nonfinite=False,
                 track_grad_norm=False):
        """params: parameters, or parameter groups (dicts: "params" plus any of lr, betas, eps, weight_decay, decoupled_weight_decay; what a
        group does not set comes from the arguments here).  Parameters that do not require a gradient are dropped from every group.
        grad_sink: the parallel.GradBucketAllReduce that owns the gradients of exactly these parameters.
        model: a SwinHPTransformerSys whose bf16 parameter copies this optimizer should keep current (optional).
        max_grad_norm: clip the gradients to this total norm (`norm_type` 2 or inf) as torch.nn.utils.clip_grad_norm_ does.
        clip_value: or clamp every gradient element to +-clip_value as torch.nn.utils.clip_grad_value_ does (not both).
        skip_nonfinite: a step whose gradients hold a NaN or an inf changes nothing and counts in `skipped_steps`; without it such
        a gradient propagates as in torch.
        track_grad_norm: measure the norms at every step (`grad_norm`, `param_grad_norms`, `guard.named_norms(model)`)."""
        if max_grad_norm is not None and clip_value is not None:
            raise ValueError("give max_grad_norm (clipping by norm) or clip_value (clipping by value), not both")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("max_grad_norm must be positive")
        if clip_value is not None and not (float(clip_value) > 0.0 and math.isfinite(float(clip_value))):
            raise ValueError("clip_value must be positive and finite")
        norm_type = _norm_kind(norm_type)
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, decoupled_weight_decay=bool(decoupled_weight_decay),
                        capturable=True, fused=True)
        params = list(params)
        if params and all(isinstance(g, dict) for g in params):  # parameter groups: own lr, betas, eps, weight_decay, decoupled_weight_decay
            groups = [dict(g, params=[p for p in g["params"] if p.requires_grad], capturable=True, fused=True) for g in params]
            if not all(g["params"] for g in groups):
                raise ValueError("a parameter group holds no parameter that requires a gradient")
        else:
            groups = [dict(params=[p for p in params if p.requires_grad])]
        params = [p for g in groups for p in g["params"]]
        if len(set(map(id, params))) != len(params):
            raise ValueError("some parameters appear in more than one parameter group")
        if set(map(id, params)) != set(map(id, grad_sink.params)):
            raise ValueError("FlatAdam and its gradient sink must be built over the same parameters")
        if len(groups) > adam_max_groups():
            raise ValueError(f"{len(groups)} parameter groups: FlatAdam steps at most {adam_max_groups()} in its one launch per bucket")
        for g in groups:
            b, e, wd = g.get("betas", betas), g.get("eps", eps), g.get("weight_decay", weight_decay)
            if len(b) != 2 or not 0.0 <= b[0] < 1.0 or not 0.0 <= b[1] < 1.0 or e < 0.0 or wd < 0.0:
                raise ValueError("invalid Adam hyper-parameters")
            if "betas" in g:
                g["betas"] = tuple(b)
            if "decoupled_weight_decay" in g:
                g["decoupled_weight_decay"] = bool(g["decoupled_weight_decay"])
        if not params or not all(p.is_cuda and p.dtype == torch.float32 for p in params):
            raise RuntimeError("FlatAdam runs on fp32 master parameters on an MI355X (HIP) device; there is no CPU path")
        self._sealed = False
        super().__init__(groups, defaults)
        self._sealed = True  # (the sink fixes the flat layout: add_param_group is for Optimizer.__init__ alone)
        self.sink = grad_sink
        self.lowp_dtype = lowp_dtype if model is not None else None
        dev = params[0].device
        self._step = torch.zeros((), dtype=torch.int64, device=dev)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.clip_value = None if clip_value is None else float(clip_value)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._skipped = torch.zeros((), dtype=torch.int64, device=dev)
        guarded = self.max_grad_norm is not None or self.clip_value is not None or self.skip_nonfinite or bool(track_grad_norm)
        self.guard = GradGuard(grad_sink, norm_type) if guarded else None
        self._flat_p, self._flat_m, self._flat_v, self._flat_lowp = [], [], [], []
        self._lowp_view = {}
        with torch.no_grad():
            for b, g in enumerate(grad_sink.buckets):
                P = torch.zeros_like(g)  # (the sink's alignment gaps: p = g = m = v = 0 stays 0 in csrc/adam.hip, also with eps = 0)
                M, V = torch.zeros_like(g), torch.zeros_like(g)
                S = torch.empty_like(g, dtype=self.lowp_dtype) if self.lowp_dtype is not None else None
                for p in grad_sink.params:
                    if grad_sink._where[p] != b:
                        continue
                    view = grad_sink._views[p]
                    off = view.storage_offset() - g.storage_offset()
                    n = p.numel()
                    pv = P[off:off + n].view_as(p)
                    pv.copy_(p)
                    p.data = pv  # the parameter now lives in the flat buffer (same values, same shape / dtype / device)
                    self.state[p] = {"step": self._step, "exp_avg": M[off:off + n].view_as(p), "exp_avg_sq": V[off:off + n].view_as(p)}
                    if S is not None:
                        self._lowp_view[id(p)] = S[off:off + n].view_as(p)
                if S is not None:
                    S.copy_(P)
                self._flat_p.append(P)
                self._flat_m.append(M)
                self._flat_v.append(V)
                self._flat_lowp.append(S)
        self._group_tables = None
        if len(self.param_groups) > 1:  # who owns which element of a bucket: static, on the device (csrc/adam.hip)
            index = {id(p): i for i, p in enumerate(grad_sink.params)}
            layout = [[] for _ in grad_sink.buckets]
            for p in grad_sink.params:
                b = grad_sink._where[p]
                layout[b].append((index[id(p)], grad_sink._views[p].storage_offset() - grad_sink.buckets[b].storage_offset(), p.numel()))
            runs, first = group_tables(layout, [[index[id(p)] for p in g["params"]] for g in self.param_groups],
                                       lengths=[f.numel() for f in grad_sink.buckets])
            self._group_tables = [(torch.tensor(r, dtype=torch.int32, device=dev).reshape(len(r), 2), torch.tensor(f, dtype=torch.int32, device=dev))
                                  for r, f in zip(runs, first)]
        self._model = model
        if model is not None:  # the model's cast cache takes its bf16 shadows from here (built at its next forward)
            model.__dict__["_shadow_provider"] = self.lowp_copy
            model.__dict__.pop("_cast_cache", None)

    def add_param_group(self, param_group):
        if getattr(self, "_sealed", False):
            raise ValueError("FlatAdam takes its parameter groups at construction: the gradient sink fixes the flat layout of parameters, "
                             "moments and ownership tables; build a new sink and optimizer over the new set of parameters")
        super().add_param_group(param_group)

    def lowp_copy(self, p, dtype):
        """The bf16 view of parameter p that `step()` keeps current, or None (other dtype / foreign parameter)."""
        return self._lowp_view.get(id(p)) if dtype == self.lowp_dtype else None

    @property
    def grad_norm(self):
        """Total gradient norm (before clipping) of the last guarded step: a 0-dim fp32 device tensor."""
        return self._guard().total_norm

    @property
    def param_grad_norms(self):
        """Per-parameter gradient norms of the last guarded step: [n_params] fp32 on the device, in the sink's parameter order."""
        return self._guard().param_norms

    @property
    def skipped_steps(self):
        """Steps `skip_nonfinite` has dropped so far: a 0-dim int64 device tensor (not part of state_dict())."""
        return self._skipped

    def _guard(self):
        if self.guard is None:
            raise RuntimeError("this FlatAdam measures no gradient norms: pass max_grad_norm, clip_value, skip_nonfinite or track_grad_norm")
        return self.guard

    def zero_grad(self, set_to_none=False):  # gradients are the sink's bucket views: zeroed in place, never detached
        self.sink.zero_grad()

    @torch.no_grad()
    def step(self, closure=None):
        if getattr(self, "_averaged_in_place", None) is not None:
            raise RuntimeError("FlatAdam.step() inside FlatWeightAverage.applied(): the parameters are the averaged weights until the block ends")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for grp in self.param_groups:
            lr = grp["lr"]
            if isinstance(lr, torch.Tensor) and not (lr.is_cuda and lr.dtype == torch.float32 and lr.numel() == 1):
                raise ValueError("a tensor learning rate must be a 0-dim float32 CUDA tensor")
        dev = self._step.device
        s = stream_ptr(dev)
        buffers = zip(self._flat_p, self.sink.buckets, self._flat_m, self._flat_v, self._flat_lowp)
        if self._group_tables is not None:
            self._step_groups(buffers, s)
            return self._stepped(loss)
        grp = self.param_groups[0]
        lr = grp["lr"]
        lr_dev = lr if isinstance(lr, torch.Tensor) else None
        b1, b2 = grp["betas"]
        hyper = (0.0 if lr_dev is not None else float(lr), ptr(lr_dev), float(b1), float(b2), float(grp["eps"]), float(grp["weight_decay"]),
                 int(grp["decoupled_weight_decay"]), ptr(self._step))
        if self.guard is None:
            for P, G, M, V, S in buffers:
                check(lib.hs_adam_step(ptr(P), ptr(G), ptr(M), ptr(V), ptr(S), P.numel(), *hyper, s), "hs_adam_step")
            check(lib.hs_adam_advance(ptr(self._step), s), "hs_adam_advance")
        else:  # measure, then step on what the device record says: clip coefficient and finite flag never visit the host
            self.guard.measure(self.max_grad_norm)
            rec, skip = ptr(self.guard.record), int(self.skip_nonfinite)
            for P, G, M, V, S in buffers:
                check(lib.hs_adam_step_guarded(ptr(P), ptr(G), ptr(M), ptr(V), ptr(S), P.numel(), *hyper, self.clip_value or 0.0, rec, skip, s),
                      "hs_adam_step_guarded")
            check(lib.hs_adam_advance_guarded(ptr(self._step), rec, skip, ptr(self._skipped), s), "hs_adam_advance_guarded")
        return self._stepped(loss)

    def _step_groups(self, buffers, s):
        """Several parameter groups: `hs_adam_step_groups`, still once per bucket -- the groups' records go by value (read here, on the
        host, at every step: a scheduler's change of `param_groups[i]["lr"]` costs no copy), ownership comes from the device tables."""
        records = _lib.adam_groups([(g["lr"], *g["betas"], g["eps"], g["weight_decay"], g["decoupled_weight_decay"]) for g in self.param_groups])
        if self.guard is None:
            for (P, G, M, V, S), (runs, first) in zip(buffers, self._group_tables):
                check(lib.hs_adam_step_groups(ptr(P), ptr(G), ptr(M), ptr(V), ptr(S), P.numel(), records, len(records), ptr(runs), runs.shape[0],
                                              ptr(first), first.numel(), P.numel(), ptr(self._step), s), "hs_adam_step_groups")
            check(lib.hs_adam_advance(ptr(self._step), s), "hs_adam_advance")
        else:  # one measurement, one clip coefficient and one finite flag for all groups
            self.guard.measure(self.max_grad_norm)
            rec, skip = ptr(self.guard.record), int(self.skip_nonfinite)
            for (P, G, M, V, S), (runs, first) in zip(buffers, self._group_tables):
                check(lib.hs_adam_step_groups_guarded(ptr(P), ptr(G), ptr(M), ptr(V), ptr(S), P.numel(), records, len(records), ptr(runs),
                                                      runs.shape[0], ptr(first), first.numel(), P.numel(), ptr(self._step), self.clip_value or 0.0,
                                                      rec, skip, s), "hs_adam_step_groups_guarded")
            check(lib.hs_adam_advance_guarded(ptr(self._step), rec, skip, ptr(self._skipped), s), "hs_adam_advance_guarded")

    def _stepped(self, loss):
        # the update went through raw pointers (no parameter `_version` moved): caches keyed by weight contents -- the bf16x3
        # splits of fp32 weights, ops._weight_split -- are told here, also for layers used outside a model's forward
        ops.RT.weight_epoch += 1
        cache = None if self._model is None else self._model.__dict__.get("_cast_cache")
        if cache is not None:
            cache.mark_refreshed_externally()
        return loss

    def load_state_dict(self, state_dict):
        """Moments and step count are COPIED into the flat buffers (the views must keep pointing there)."""
        own = {id(p): st for p, st in self.state.items()}
        keep = {id(p): dict(st) for p, st in self.state.items()}
        decoupled = [g["decoupled_weight_decay"] for g in self.param_groups]
        super().load_state_dict(state_dict)  # (torch's layout: parameter ids numbered through the groups, options restored per group)
        for g, own_decoupled in zip(self.param_groups, decoupled):
            g.setdefault("decoupled_weight_decay", own_decoupled)  # (a state dict of an optimizer without that option)
            g["capturable"] = g["fused"] = True
        with torch.no_grad():
            step = None
            for p in (p for g in self.param_groups for p in g["params"]):
                new, old = self.state.get(p, {}), keep[id(p)]
                for k in ("exp_avg", "exp_avg_sq"):
                    if k not in new:
                        old[k].zero_()  # an optimizer that never stepped: torch would start from zero moments
                    elif new[k] is not old[k]:
                        old[k].copy_(new[k])
                if "step" in new and new["step"] is not old["step"]:
                    step = new["step"]
                self.state[p] = own[id(p)]
                self.state[p].update(old)
            # no step count in the loaded state = a state that never stepped: moments (zeroed above) and bias correction agree
            self._step.fill_(int(float(step)) if step is not None else 0)
        ops.RT.weight_epoch += 1


_AVG_KINDS = {"swa": 0, "ema": 1}


class FlatWeightAverage:
    """A running average of a FlatAdam's parameters, kept in flat buffers next to them: torch.optim.swa_utils.AveragedModel without the
    second module.

        avg = FlatWeightAverage(opt, "ema", decay=0.999)       # updated at the end of every opt.step(), also under graph replay
        avg = FlatWeightAverage(opt, "swa")                    # avg.update() once per epoch, from the trainer's swa_epoch_start on
        with avg.applied():                                    # the model IS the averaged model inside: validate, export
            validate(model)
        avg.copy_to_model()                                    # the end of an SWA run

    kind "swa": the equal average of AveragedModel's default (`avg += (p - avg) / (n_averaged + 1)`); "ema": `avg = decay * avg +
    (1 - decay) * p` (`get_ema_multi_avg_fn(decay)`).  The first update copies the parameters.  Both are ATen's lerp in fp32, one
    `hs_weight_avg_update` launch per bucket; `n_averaged` is a 0-dim int64 DEVICE tensor the kernels read and `hs_weight_avg_advance`
    increments, so `update()` allocates nothing, never synchronises and is capturable.  With a `skip_nonfinite` optimizer an update follows
    the guard record of the last step: a skipped step is not averaged.
    every_step: register `update` as a step post-hook of the optimizer (None: True for "ema", False for "swa"); `detach()` removes it.
    model: the module whose bf16 parameter copies must follow a swap (default: the optimizer's `model=`).
    The model has only LayerNorms and constant buffers: there is no `update_bn` and no buffer averaging to do."""

    def __init__(self, optimizer, kind="swa", decay=0.999, every_step=None, model=None):
        if not isinstance(optimizer, FlatAdam):
            raise ValueError("FlatWeightAverage averages the flat parameter buffers of a heal_swin_amd.optim.FlatAdam")
        if kind not in _AVG_KINDS:
            raise ValueError(f"kind must be 'swa' or 'ema', got {kind!r}")
        if not 0.0 <= float(decay) <= 1.0:
            raise ValueError("decay must be in [0, 1]")
        self.optimizer, self.kind, self.decay = optimizer, kind, float(decay)
        self._model = model if model is not None else optimizer._model
        self.n_averaged = torch.zeros((), dtype=torch.int64, device=optimizer._step.device)
        self._flat_avg = [torch.zeros_like(P) for P in optimizer._flat_p]  # (the alignment gaps: p = 0 there, so avg stays 0)
        self._view = {}
        sink = optimizer.sink
        for p in sink.params:
            b = sink._where[p]
            off = sink._views[p].storage_offset() - sink.buckets[b].storage_offset()
            self._view[id(p)] = self._flat_avg[b][off:off + p.numel()].view_as(p)
        self._hook = None
        if (kind == "ema") if every_step is None else every_step:
            self._hook = optimizer.register_step_post_hook(lambda *a, **k: self.update())

    def of(self, p):
        """The average of parameter p: a view into the flat buffer (same shape as p)."""
        return self._view[id(p)]

    def detach(self):
        """Stop following the optimizer's steps (`every_step`)."""
        if self._hook is not None:
            self._hook.remove()
            self._hook = None

    def _refuse_inside_applied(self, what):
        if getattr(self.optimizer, "_averaged_in_place", None) is not None:
            raise RuntimeError(f"FlatWeightAverage.{what} inside applied(): parameters and average have changed places until the block ends")

    @torch.no_grad()
    def update(self):
        """Take the optimizer's parameters as they are now into the average (on the current stream)."""
        self._refuse_inside_applied("update()")
        opt = self.optimizer
        guarded = opt.guard is not None and opt.skip_nonfinite
        rec, skip = (ptr(opt.guard.record) if guarded else None), int(guarded)
        s, count = stream_ptr(self.n_averaged.device), ptr(self.n_averaged)
        for A, P in zip(self._flat_avg, opt._flat_p):
            check(lib.hs_weight_avg_update(ptr(A), ptr(P), P.numel(), _AVG_KINDS[self.kind], self.decay, count, rec, skip, s), "hs_weight_avg_update")
        check(lib.hs_weight_avg_advance(count, rec, skip, s), "hs_weight_avg_advance")

    def _parameters_changed(self):
        # as FlatAdam._stepped: the parameters changed through raw pointers.  The bf16 copies FlatAdam owns were written with them;
        # a cast cache with copies of its own (or an optimizer without a model) has to re-make them at the next forward
        ops.RT.weight_epoch += 1
        cache = None if self._model is None else self._model.__dict__.get("_cast_cache")
        if cache is not None:
            if self.optimizer.lowp_dtype is not None and cache.all_external:
                cache.mark_refreshed_externally()
            else:
                cache.invalidate()

    def _swap(self):
        opt = self.optimizer
        s = stream_ptr(self.n_averaged.device)
        for P, A, S in zip(opt._flat_p, self._flat_avg, opt._flat_lowp):
            check(lib.hs_weight_avg_swap(ptr(P), ptr(A), ptr(S), P.numel(), s), "hs_weight_avg_swap")
        self._parameters_changed()

    @contextlib.contextmanager
    def applied(self):
        """Inside, the model's parameters (and the optimizer's bf16 copies of them) are the averaged weights and `of(p)` holds the trained
        ones: one `hs_weight_avg_swap` per bucket on the way in, one on the way out -- also when the block raises.  Two swaps restore
        every bit.  `optimizer.step()` and `update()` inside raise RuntimeError."""
        self._refuse_inside_applied("applied()")
        with torch.no_grad():
            self._swap()
        self.optimizer._averaged_in_place = self
        try:
            yield self
        finally:
            self.optimizer._averaged_in_place = None
            with torch.no_grad():
                self._swap()

    @torch.no_grad()
    def copy_to_model(self):
        """The end of an SWA run: parameters and their bf16 copies become the average (which is kept)."""
        self._refuse_inside_applied("copy_to_model()")
        for P, A, S in zip(self.optimizer._flat_p, self._flat_avg, self.optimizer._flat_lowp):
            P.copy_(A)
            if S is not None:
                S.copy_(A)
        self._parameters_changed()

    def state_dict(self):
        """kind, decay, n_averaged (an int: SYNCHRONISES) and a copy of every parameter's average, in the sink's parameter order."""
        return {"kind": self.kind, "decay": self.decay, "n_averaged": int(self.n_averaged),
                "averages": [self.of(p).detach().clone() for p in self.optimizer.sink.params]}

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """The averages are COPIED into the flat buffers (the views keep pointing there); kind must match, decay is taken over."""
        params = self.optimizer.sink.params
        averages = state_dict["averages"]
        if state_dict["kind"] != self.kind:
            raise ValueError(f"the state holds a {state_dict['kind']!r} average, this is {self.kind!r}")
        if not 0.0 <= float(state_dict["decay"]) <= 1.0:
            raise ValueError("decay must be in [0, 1]")
        if len(averages) != len(params) or any(a.shape != p.shape for a, p in zip(averages, params)):
            raise ValueError("the state holds the averages of other parameters")
        self._refuse_inside_applied("load_state_dict()")
        self.decay = float(state_dict["decay"])
        for a, p in zip(averages, params):
            self.of(p).copy_(a)
        self.n_averaged.fill_(int(state_dict["n_averaged"]))
