"""The fp8 mode tests (tests/test_fp8_modes_gpu.py) cover what the product launches: every fp8-weight (w8) and block-scaled (mx) row
of tests/golden/epilogue_census_fp8.json, the census of the flagship DDIM step built with fp8 weights and with fp8 weights + MX
(tools/epilogue_census.py --weight-bits 8 [--act-bits 8], recorded on an MI355X), is matched by a case of FP8_MODE_CASES on its
(form, tile, split-K > 1, flags).  From the table and the JSON alone: no device call."""
import json
import os

import pytest

from tests.fp8_mode_cases import (FP8_MODE_CASES, LN_FOLD, GN_MODES, MODES, MX_TILES, W8_TILES, case_id, census_key, covered_keys, flags_of,
                                  geglu_capable, res_rows_of, tile_table)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "epilogue_census_fp8.json")
PARTS = ("fp8_step", "fp8_mx_step")


def census():
    return json.load(open(GOLDEN))


def fp8_rows():
    c = census()
    return [(part, r) for part in PARTS for r in c[part] if r["form"] in ("w8", "mx")]


def row_id(pr):
    part, r = pr
    return f"{part}-{r['form']}-t{r['tile']}-sk{r['splitk']}-{r['mode']}"


def test_census_file_is_what_the_tool_writes():
    c = census()
    assert "tools/epilogue_census.py --weight-bits 8" in c["_how"]
    names = {t: None for t, _, _, _ in tile_table()}
    for part in PARTS:
        assert c[part], part
        for r in c[part]:
            assert set(r) == {"tile", "name", "splitk", "form", "kind", "mode", "flags", "launches"}, r
            assert r["tile"] in names and r["form"] in ("plain", "ups", "w8", "mx", "multi"), r
            assert r["form"] not in ("w8", "mx") or r["kind"] == 0, f"the fp8 forms exist as the generic staged kernel only: {r}"
    assert any(r["form"] == "w8" for r in c["fp8_step"]) and not any(r["form"] == "mx" for r in c["fp8_step"])
    assert any(r["form"] == "mx" for r in c["fp8_mx_step"]) and any(r["form"] == "w8" for r in c["fp8_mx_step"])


@pytest.mark.parametrize("part_row", fp8_rows(), ids=row_id)
def test_census_row_has_a_case(part_row):
    part, r = part_row
    key = census_key(r["form"], r["tile"], r["splitk"], r["flags"])
    assert key in covered_keys(), f"{part}: no case of FP8_MODE_CASES launches form {r['form']} on tile {r['tile']} ({r['name']}) " \
                                  f"{'split-K' if r['splitk'] > 1 else 'unsplit'} with flags {r['flags']} ({r['mode']})"


def test_census_tiles_have_the_operand_form():
    for _, r in fp8_rows():
        assert r["tile"] in (W8_TILES if r["form"] == "w8" else MX_TILES), r


def test_no_block_scaled_launch_carries_the_layernorm_fold():
    """Fp8State::use_mx leaves LayerNorm-fold launches on fp16 activations (profiles/mx_ln_fold_error.json): the step has none on the MX form,
    and the fold still runs (on the fp8-weight or fp16 form)"""
    rows = census()["fp8_mx_step"]
    assert not [r for r in rows if r["form"] == "mx" and r["flags"] & LN_FOLD]
    assert [r for r in rows if r["form"] != "mx" and r["flags"] & LN_FOLD]


def test_table_shape():
    """every tile with the instantiation, every mode unsplit and (where the mode has a split form) split, unique ids"""
    ids = [case_id(c) for c in FP8_MODE_CASES]
    assert len(set(ids)) == len(ids)
    assert W8_TILES and MX_TILES
    for form, tiles in (("w8", W8_TILES), ("mx", MX_TILES)):
        modes = {c.mode for c in FP8_MODE_CASES if c.form == form}
        assert {"stats", "stats_res", "ln", "ln_geglu", "res_rows_half", "res_rows_mid", "scale_res"} <= modes, (form, modes)
        for t in tiles:
            for mode in modes:
                if mode == "ln_geglu" and not geglu_capable(t):
                    continue
                mine = [c for c in FP8_MODE_CASES if (c.form, c.tile, c.mode) == (form, t, mode)]
                assert any(c.splitk == 1 for c in mine), (form, t, mode)
                assert any(c.splitk > 1 for c in mine) == (MODES[mode][1] is not None or mode in GN_MODES), (form, t, mode)
    assert set(GN_MODES) <= {c.mode for c in FP8_MODE_CASES if c.form == "w8"}
    for c in FP8_MODE_CASES:
        assert c.mode in MODES and (flags_of(c) is not None or c.splitk > 1), c
    assert any(c.mode == "conv_b2" and c.splitk > 1 for c in FP8_MODE_CASES)
    # the residual of res_rows rows: m / 2, and a value strictly between m / 2 and m
    for m in {c.shape[0] for c in FP8_MODE_CASES if c.mode.startswith("res_rows")}:
        assert res_rows_of("res_rows_half", m) * 2 == m and m // 2 < res_rows_of("res_rows_mid", m) < m, m
