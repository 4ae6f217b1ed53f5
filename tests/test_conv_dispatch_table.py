"""The conv dispatch answers what it answered at the commit tests/golden/conv_dispatch.json was recorded from (host code only:
the library loads without a device and no query dereferences a pointer).  The sweep and the queries are those of
tools/conv_dispatch_table.py; the table is never regenerated from a library whose dispatch has since been reworked."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN, ROOT

_spec = importlib.util.spec_from_file_location("conv_dispatch_table", os.path.join(ROOT, "tools", "conv_dispatch_table.py"))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)

COL = {c: i for i, c in enumerate(T.COLUMNS)}
NAMES = {"smallco_fwd", "head_fwd_kernel", "convbf_kernel", "wino4_kernel", "wino_kernel", "conv3x3_kernel", "igemm_kernel<fwd>",
         "head_dgrad_kernel", "smallci_dgrad", "igemm_kernel<dgrad>",
         "smallco_wgrad", "head_wgrad_kernel", "wgradb_kernel", "winow4_kernel", "winow_kernel", "wgrad4d_kernel",
         "wgrad3x3_kernel", "smallci_wgrad_kernel", "igemm_kernel<wgrad>"}


@pytest.fixture(scope="module")
def stored():
    path = os.path.join(GOLDEN, "conv_dispatch.json")
    assert os.path.getsize(path) < 256 * 1024
    with open(path) as f:
        return json.load(f)


def test_dispatch_answers_equal_the_stored_table(stored):
    table, labels = T.build_table()
    diffs = T.first_differences(stored, table, labels, limit=1)
    assert not diffs, "first difference: %s: %s: stored %r, now %r" % diffs[0]
    assert len(table["rows"]) == len(stored["rows"]) and table["index"] == stored["index"]


def test_stored_table_covers_every_family_and_is_consistent(stored):
    rows = stored["rows"]
    variants = ["fwd", "fwd_stats", "dgrad", "dgrad_stats", "wgrad", "wgrad_stats"]
    seen = {r[COL[c]].split(":")[0] for r in rows for c in variants}
    assert seen == NAMES, (seen ^ NAMES)                    # all 19 names the library can report, and no "invalid"
    for r in rows:
        # a descriptor's two forward routes differ only where a kernel that computes no statistics takes the call without them
        if r[COL["fwd"]] != r[COL["fwd_stats"]]:
            assert r[COL["fwd"]] in ("smallco_fwd", "head_fwd_kernel"), r
        assert r[COL["dgrad"]] == r[COL["dgrad_stats"]] and r[COL["wgrad"]] == r[COL["wgrad_stats"]], r
        # every call that has a kernel has its formats
        for io, c in (("io0", "fwd"), ("io1", "dgrad"), ("io2", "wgrad")):
            if r[COL[c]] != "invalid":
                assert r[COL[io]][0] == 0, r
