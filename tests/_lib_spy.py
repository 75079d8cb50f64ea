"""Census of the C entry points a call runs, shared by the launch-census assertions of tests/test_gpu_seg_step.py,
tests/test_gpu_depth_loss.py and tests/test_gpu_depth_step.py: the name `lib` of the given modules is replaced by a recorder
that passes every call on to the real library."""


def spy_on(monkeypatch, prefixes, modules):
    """Record, in call order, the names of the `hs_*` entry points that start with one of `prefixes` and are reached through the
    name `lib` of one of `modules` (heal_swin_amd._lib itself for the modules that import the name at call time).  Returns the
    list the names are appended to; monkeypatch undoes the substitution at the end of the test."""
    from heal_swin_amd import _lib
    real, called = _lib.lib, []
    prefixes = tuple(prefixes)

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name.startswith(prefixes):
                def wrap(*a):
                    called.append(name)
                    return fn(*a)
                return wrap
            return fn

    for mod in modules:
        monkeypatch.setattr(mod, "lib", Spy())
    return called


def launches(called):
    """The recorded names without the host-side queries (`*_supported`, `*_blocks`, `*_partials`), sorted."""
    return sorted(c for c in called if not c.endswith(("_supported", "_blocks", "_partials")))
