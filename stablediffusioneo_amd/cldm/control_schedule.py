"""Control schedule: per sampling step and per control network, whether the network acts on both halves of the classifier-free
guidance pair, on the conditional half only, or not at all (include/sdeo.h: sdeo_set_control_mode).

    model.control_schedule = ControlSchedule(start=0.0, end=0.5)               # one window for every net
    model.control_schedule = [ControlSchedule(on="cond"), ControlSchedule(0.0, 0.5)]   # one entry per net

A net is active at loop step i of S (i = 0 is the first, noisiest step) when the step lies wholly inside its window,

    i / S >= start   and   (i + 1) / S <= end,

and runs in its `on` mode then ("both", or "cond": the conditional half only -- the reference's guess mode, whose unconditional half
runs without ControlNet, `canny2image_torch.py:48`); outside the window it is off.  The window rule is the one diffusers documents for
`control_guidance_start` / `control_guidance_end` ("the percentage of total steps at which the ControlNet starts / stops applying"),
written down from memory of that pipeline: it is this module's own definition and is NOT pinned to diffusers' code.  A1111's "starting
/ ending control step" names the same two numbers.

`model.control_schedule = None` (the default) changes nothing anywhere.  A schedule acts when the request can take the fused path:
conditioning that carries the hints on both sides, or no guidance at all (then there is no second half: "cond" means "both").  A
request whose unconditional conditioning has `c_concat = None` keeps the two-call route it always had, schedule or not."""
from __future__ import annotations

import contextlib
from typing import List, Optional, Tuple

# the modes of include/sdeo.h (SDEO_CONTROL_*); restated so that this module imports without the library (tests hold them equal)
BOTH, COND, OFF = 0, 1, 2
_ON = {"both": BOTH, "cond": COND}


class ControlSchedule:
    """the window [start, end] (fractions of the sampling run, 0 <= start < end <= 1) and the mode (`on`: "both" or "cond") of one net"""

    def __init__(self, start: float = 0.0, end: float = 1.0, on: str = "both"):
        for name, v in (("start", start), ("end", end)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v:
                raise ValueError(f"ControlSchedule: {name} must be a number, got {v!r}")
        start, end = float(start), float(end)
        if not 0.0 <= start < end <= 1.0:
            raise ValueError(f"ControlSchedule: need 0 <= start < end <= 1, got start = {start}, end = {end}")
        if on not in _ON:
            raise ValueError(f"ControlSchedule: on must be 'both' or 'cond', got {on!r}")
        self.start, self.end, self.on = start, end, on

    def mode_at(self, i: int, S: int) -> int:
        """this net's mode at loop step i of S.  The two comparisons are made on integers scaled by S, i >= start * S and i + 1 <= end * S,
        with start * S / end * S rounded to the nearest integer when they are within 1e-9 of one (0.25 * 20 is 5, whatever the
        floating-point product says)"""
        i, S = int(i), int(S)
        if S < 1 or not 0 <= i < S:
            raise ValueError(f"ControlSchedule.mode_at: step {i} of {S}")
        lo, hi = _snap(self.start * S), _snap(self.end * S)
        return _ON[self.on] if i >= lo and i + 1 <= hi else OFF

    def key(self) -> Tuple[float, float, str]:
        return (self.start, self.end, self.on)

    def __repr__(self):
        return f"ControlSchedule(start={self.start}, end={self.end}, on={self.on!r})"

    def __eq__(self, other):
        return isinstance(other, ControlSchedule) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())


def _snap(v: float) -> float:
    r = round(v)
    return float(r) if abs(v - r) < 1e-9 else v


def normalize(schedule, nets: int) -> Optional[List[ControlSchedule]]:
    """`schedule` as a list of one ControlSchedule per net: None stays None, one ControlSchedule serves every net, a sequence must hold
    exactly `nets` of them"""
    if schedule is None:
        return None
    if isinstance(schedule, ControlSchedule):
        return [schedule] * int(nets)
    if not isinstance(schedule, (list, tuple)) or not all(isinstance(s, ControlSchedule) for s in schedule):
        raise ValueError(f"control_schedule: expected None, a ControlSchedule or a list of them, got {schedule!r}")
    if len(schedule) != int(nets):
        raise ValueError(f"control_schedule: {len(schedule)} entries for {int(nets)} control networks")
    return list(schedule)


def modes_at(schedule, i: int, S: int, nets: Optional[int] = None) -> Tuple[int, ...]:
    """each net's mode at loop step i of S; `schedule` one ControlSchedule or a list with one per net (nets: how many, for one)"""
    sch = normalize(schedule, nets if nets is not None else (len(schedule) if isinstance(schedule, (list, tuple)) else 1))
    return tuple(s.mode_at(i, S) for s in sch)


def schedule_key(schedule) -> Optional[tuple]:
    """what a captured loop bakes in of the schedule (part of the samplers' `shape_key`)"""
    if schedule is None:
        return None
    return tuple(s.key() for s in ([schedule] if isinstance(schedule, ControlSchedule) else schedule))


def step_plan(model, applies: bool, unguided: bool, S: int) -> Optional[List[Tuple[int, ...]]]:
    """The modes of every net at every step of an S-step run of `model` under its `control_schedule`, or None when nothing is to be
    set: no schedule, or a request that does not take the fused path (`applies`).  unguided: there is no second half, COND is BOTH."""
    schedule = getattr(model, "control_schedule", None)
    if schedule is None or not applies:
        return None
    rt = getattr(model, "rt", None)
    if rt is None or not getattr(rt, "control_modes", False):
        raise RuntimeError("model.control_schedule is set but the runtime has no control modes: create_model(..., control_modes=True)")
    sch = normalize(schedule, 1 + rt.extra_controlnets)
    plan = [tuple(s.mode_at(i, S) for s in sch) for i in range(int(S))]
    if unguided:
        plan = [tuple(BOTH if m == COND else m for m in row) for row in plan]
    return plan


@contextlib.contextmanager
def step_modes(model, plan, i: int):
    """`with step_modes(model, plan, i): <the library call of step i>` -- the modes of step i are handed to the runtime before the call
    (an eager step, a per-step call, a step being captured: the library reads them when the call launches) and every net is back in
    BOTH when the block is left, by return or by exception: nothing a run sets outlives its step, so what follows without a schedule
    runs as it always did.  plan None: nothing is touched."""
    if plan is None:
        yield
        return
    model.rt.set_control_modes(plan[i])
    try:
        yield
    finally:
        model.rt.set_control_modes(None)
