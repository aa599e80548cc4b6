"""Control schedule without a GPU: the window rule against a hand-written table, validation, the new symbols and constants of
include/sdeo.h, the opt-in (no schedule, no enabled handle), and the condition the GPU parity tests of tests/test_control_schedule_gpu.py
stand on: at their shapes, hints and scales the oracle's controlled and uncontrolled eps differ by at least 5 x the parity bound."""
import ctypes as C
import inspect

import pytest
import torch

from stablediffusioneo_amd.cldm import control_schedule as CS
from stablediffusioneo_amd.cldm.control_schedule import BOTH, COND, OFF, ControlSchedule
from tests import control_schedule_cases as CC

# steps at which a net with window (start, end) is on, for S = 4, 5, 20: written by hand from  i / S >= start and (i + 1) / S <= end
ON_STEPS = {
    (4, 0.0, 1.0): [0, 1, 2, 3],
    (4, 0.0, 0.5): [0, 1],
    (4, 0.25, 0.75): [1, 2],
    (4, 0.5, 1.0): [2, 3],
    (5, 0.0, 1.0): [0, 1, 2, 3, 4],
    (5, 0.0, 0.5): [0, 1],              # step 2 covers [0.4, 0.6]: it ends after 0.5
    (5, 0.25, 0.75): [2],               # step 1 starts at 0.2 < 0.25, step 3 ends at 0.8 > 0.75
    (5, 0.5, 1.0): [3, 4],              # step 2 starts at 0.4 < 0.5
    (20, 0.0, 1.0): list(range(20)),
    (20, 0.0, 0.5): list(range(10)),
    (20, 0.25, 0.75): list(range(5, 15)),
    (20, 0.5, 1.0): list(range(10, 20)),
}


@pytest.mark.parametrize("S_,start,end", sorted(ON_STEPS))
@pytest.mark.parametrize("on", ["both", "cond"])
def test_modes_at_against_the_table(S_, start, end, on):
    sch = ControlSchedule(start, end, on)
    want_on = {"both": BOTH, "cond": COND}[on]
    want = [want_on if i in ON_STEPS[(S_, start, end)] else OFF for i in range(S_)]
    assert [sch.mode_at(i, S_) for i in range(S_)] == want
    assert [CS.modes_at(sch, i, S_) for i in range(S_)] == [(m,) for m in want]
    # a list: one entry per net, each under its own window
    other = ControlSchedule(0.0, 1.0, "both")
    assert [CS.modes_at([sch, other], i, S_) for i in range(S_)] == [(m, BOTH) for m in want]


def test_validation():
    for start, end in ((-0.1, 1.0), (0.0, 1.1), (0.5, 0.5), (0.6, 0.4), (float("nan"), 1.0), ("0", 1.0), (0.0, None)):
        with pytest.raises(ValueError, match="ControlSchedule"):
            ControlSchedule(start, end)
    with pytest.raises(ValueError, match="'both' or 'cond'"):
        ControlSchedule(on="uncond")
    with pytest.raises(ValueError, match="step 4 of 4"):
        ControlSchedule().mode_at(4, 4)
    a = ControlSchedule(0.0, 0.5, "cond")
    assert CS.normalize(None, 2) is None
    assert CS.normalize(a, 2) == [a, a]
    with pytest.raises(ValueError, match="1 entries for 2 control networks"):
        CS.normalize([a], 2)
    with pytest.raises(ValueError, match="expected None, a ControlSchedule or a list"):
        CS.normalize([a, (0.0, 1.0)], 2)
    assert CS.schedule_key(None) is None
    assert CS.schedule_key(a) == ((0.0, 0.5, "cond"),) and CS.schedule_key([a, ControlSchedule()]) == ((0.0, 0.5, "cond"), (0.0, 1.0, "both"))
    assert ControlSchedule(0, 1) == ControlSchedule(0.0, 1.0, "both") and ControlSchedule(0, 1) != ControlSchedule(0, 1, "cond")


def test_new_symbols_and_constants():
    from stablediffusioneo_amd import _lib
    lib = _lib.load()
    names = _lib.declared_symbols()
    I, V = C.c_int, C.c_void_p
    for n, args in {"sdeo_enable_control_modes": [V], "sdeo_set_control_mode": [V, I, I]}.items():
        assert n in names and hasattr(lib, n), n
        assert getattr(lib, n).restype is I and list(getattr(lib, n).argtypes) == args, n
    assert [_lib.header_constant("SDEO_CONTROL_" + n) for n in ("BOTH", "COND", "OFF")] == [0, 1, 2] == [BOTH, COND, OFF]
    assert lib.sdeo_version() == 101 == _lib.header_constant("SDEO_ABI_VERSION")
    # the entry points the modes act in keep their prototypes
    assert list(lib.sdeo_apply_model.argtypes) == [V, V, V, V, V, V, I, I, V, V]
    null = C.c_void_p(0)
    for call, msg in ((lambda: lib.sdeo_enable_control_modes(null), "sdeo_enable_control_modes: null handle"),
                      (lambda: lib.sdeo_set_control_mode(null, 0, 0), "sdeo_set_control_mode: null handle")):
        assert call() != 0
        assert msg in lib.sdeo_last_error().decode()


def test_no_schedule_builds_no_enabled_handle(monkeypatch):
    """the feature is opt-in at every layer: the defaults are off, and a pipeline initialised without a schedule asks create_model for a
    plain runtime (one with a schedule asks for control modes)"""
    from stablediffusioneo_amd import canny2image, hed2image, multi2image, scribble2image
    from stablediffusioneo_amd.cldm import cldm, model
    from stablediffusioneo_amd.runtime import SdeoRuntime
    assert inspect.signature(SdeoRuntime.__init__).parameters["control_modes"].default is False
    assert inspect.signature(model.create_model).parameters["control_modes"].default is False
    assert cldm.ControlLDM.control_schedule is None
    for mod in (canny2image, hed2image, multi2image, scribble2image):
        assert inspect.signature(mod.hackathon.initialize).parameters["control_schedule"].default is None
    # the pinned `process` signatures do not know the feature
    assert "control_schedule" not in inspect.signature(canny2image.hackathon.process).parameters

    class Asked(Exception):
        pass

    def fake_create_model(*args, **kwargs):
        raise Asked(kwargs)

    monkeypatch.setattr(canny2image, "create_model", fake_create_model)
    for schedule, want in ((None, False), (ControlSchedule(on="cond"), True)):
        with pytest.raises(Asked) as e:
            canny2image.hackathon().initialize(config="tiny", apply_canny=lambda *a: None, control_schedule=schedule)
        assert e.value.args[0]["control_modes"] is want
    with pytest.raises(ValueError, match="2 entries for 1 control networks"):       # checked before anything is built
        canny2image.hackathon().initialize(config="tiny", apply_canny=lambda *a: None, control_schedule=[ControlSchedule(), ControlSchedule()])


@pytest.mark.parametrize("index", [0, 1, 2, -1])
def test_parity_inputs_can_tell_a_dropped_control(index):
    """K = 1 and K = 2 at the GPU tests' inputs and scales (index -1: the per-conv configuration): dropping the control of any one net
    moves eps by at least 5 x REL_MAX of its scale, image by image -- so a COND / OFF result that kept, or lost, a control it should
    not have cannot pass the parity bound"""
    for what, i, gap in CC.can_tell(index):
        print(f"[control-schedule] case {index} image {i} {what}: {gap:.3f} of the scale")
        assert gap >= 5 * CC.REL_MAX, (what, i)
    # `expected` composes per image: COND on net 0 alone is net 0's eps on the first half and the uncontrolled eps on the second
    r, n = CC.refs(index), CC.refs(index)["none"].shape[0]
    e = CC.expected(index, (COND,))
    assert torch.equal(e[: n // 2], r["net0"][: n // 2]) and torch.equal(e[n // 2:], r["none"][n // 2:])
    assert torch.equal(CC.expected(index, (OFF, BOTH)), r["net1"]) and torch.equal(CC.expected(index, (BOTH, BOTH)), r["both"])
