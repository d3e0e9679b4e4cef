"""GPU (-m gpu): which kernels a form of the step launches, and how often.

cfx_step is a sequence of launches chosen by layout, form, pending commit and the way the spawn records travel; the parity
tests pin what the sequence computes, this file pins the sequence itself: the symbol the engine reports for every timing
slot (`_profile_symbols`) and the launches counted in it (`_profile_read`) over 20 profiled steps of the stock 6x6 grid,
for every entry of test_reference_forms.FORMS, the lane-change step, and an engine that tracks lane flow (whose commit is a
launch of its own).  The table was read from the library before cfx_step was split into its parts, and agrees with a
reading of that code; one entry differs from what that library reported: `ring-own-commit` (form digit 4) walked the lanes
with the wave-granular kernel that has been removed since, and now runs kr_action<256> like every other lane-walking form.

A slot's symbol is that of the kernel launched LAST in it, profiled or not: the `kr_commit` of the deferred-commit forms is
the launch `sync()` sends out before profiling starts — their profiled steps count none."""
import json

import pytest

from conftest import SHADOW_GPU, assert_hip_backend
from test_reference_forms import FORMS

pytestmark = pytest.mark.gpu

SLOTS = ("k_spawn_link", "k_admit", "k_action", "k_cross", "k_scan", "k_scatter", "k_halo_export", "k_halo_import", "k_commit")


def _row(admit, action, cross, scan=("", 0), scatter=("", 0), commit=("", 0)):
    return dict(zip(SLOTS, (("", 0), admit, action, cross, scan, scatter, ("", 0), ("", 0), commit)))


_RING_MERGED = dict(admit=("kr_admit<true>", 20), commit=("kr_commit", 0))    # the commit rides with the next admission
_RING_COMMIT = dict(admit=("kr_admit<false>", 20), commit=("kr_commit", 20))  # the commit is a launch of its own
_LIST = dict(action=("kl_action", 20), scan=("kr_index", 20))
_DENSE = dict(action=("kd_action", 20), scan=("k_scan", 20), scatter=("k_scatter<false>", 20))

LAUNCHES = {
    "auto": _row(action=("kr_action<256>", 20), cross=("kr_cross", 20), **_RING_MERGED),
    "ring-block-latency": _row(action=("kr_action<256>", 20), cross=("kr_cross", 20), **_RING_MERGED),
    "ring-list-throughput": _row(cross=("k_cross2<false, RingCtx, RingOut>", 20), **_LIST, **_RING_MERGED),
    "ring-list-latency": _row(cross=("kr_cross", 20), **_LIST, **_RING_MERGED),
    "ring-list-ticket": _row(cross=("k_cross2<false, RingCtx, RingOut>", 20), **_LIST, **_RING_MERGED),
    "ring-own-commit": _row(action=("kr_action<256>", 20), cross=("kr_cross", 20), **_RING_COMMIT),
    "dense-round2": _row(admit=("kd_admit<false, kAdmitRecs>", 20), cross=("k_cross<false>", 20), **_DENSE),
    "dense-lanes-bigbatch": _row(admit=("kd_admit<true, kAdmitRecs>", 20), cross=("k_cross2<false>", 20), **_DENSE),
    "dense-lanes": _row(admit=("kd_admit<true, kAdmitRecs>", 20), cross=("k_cross<false>", 20), **_DENSE),
    "lane-change": _row(admit=("k_admit", 20), action=("k_action<true>", 20), cross=("k_cross<true>", 20), scan=("k_scan", 20),
                        scatter=("k_scatter<true>", 20)),
    "lane-flow": _row(action=("kr_action<256>", 20), cross=("kr_cross", 20), **_RING_COMMIT),
}


def _config(scen, workdir, name, tag, **top):
    base = scen.materialize(name, workdir)
    if not top:
        return base
    c = json.load(open(base))
    c.update(top)
    out = base.replace(".json", "_launches_%s.json" % tag)
    with open(out, "w") as f:
        json.dump(c, f)
    return out


def test_the_table_covers_every_form():
    assert set(LAUNCHES) == set(FORMS) | {"lane-change", "lane-flow"}


@pytest.mark.parametrize("case", sorted(LAUNCHES))
def test_step_launches(mod, scen, workdir, case):
    if SHADOW_GPU:
        pytest.skip("about the device library's launches: the twin has none")
    top = {"laneChange": True} if case == "lane-change" else {"cfx": FORMS[case]} if FORMS.get(case) else {}
    eng = mod.Engine(_config(scen, workdir, "grid_6x6", case, **top), 1)
    assert_hip_backend(eng)
    if case == "lane-flow":
        eng.track_lane_flow(True)
    for _ in range(12):
        eng.next_step()
    eng.sync()
    eng._profile_enable(True)
    for _ in range(20):
        eng.next_step()
    prof, syms = eng._profile_read(), eng._profile_symbols()
    got = {k: (syms.get(k, ""), prof[k][1]) for k in prof}
    assert got == LAUNCHES[case], case


@pytest.mark.parametrize("value", [10000, 50000])
def test_form_digits_that_name_no_form_are_rejected(mod, scen, workdir, value):
    if SHADOW_GPU:
        pytest.skip("about the device library's cfx_create: the twin ignores the knob")
    cfg = _config(scen, workdir, "example_1x1", "reject%d" % value, cfx={"ringLanesPerWave": value})
    with pytest.raises(RuntimeError, match=r"ringLanesPerWave = %d" % value):
        mod.Engine(cfg, 1)
