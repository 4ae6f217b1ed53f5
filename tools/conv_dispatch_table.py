"""The conv dispatch's answers over a fixed sweep of descriptors, as a table that a refactor of the dispatch must reproduce.

For every descriptor of the sweep the library is asked, on the host alone (no device is touched, no pointer is dereferenced):
avsep_conv_kernel_variant for modes 0/1/2 with and without statistics, avsep_conv_io_formats for modes 0/1/2,
avsep_conv_packed_floats for modes 0/1, the four *_workspace_bytes queries, avsep_conv2d_head_applicable and
avsep_conv2d_dgrad_act_fused.  The stored table (tests/golden/conv_dispatch.json) holds the distinct answer rows and, per
descriptor in sweep order, the index of its row.

The sweep is written out below, not derived from running the model: the conv geometries of the full-size step (unet7 with
ngf 64 on 256x256 spectrograms, the dilated ResNet-18 trunk on 224x224 frames), a few maps the kernels tile raggedly, and one
plain few-output-channel conv, each crossed with batch, precision, planned batch and every single AVSEP_ALGO_NO_* bit.

Usage: python tools/conv_dispatch_table.py [--table FILE]            print the differences against the stored table
       python tools/conv_dispatch_table.py [--table FILE] --write    store the table (only ever from the commit whose
                                                                      dispatch is the reference, never from a refactored one)"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
TABLE = os.path.join(ROOT, "tests", "golden", "conv_dispatch.json")

ACT_NONE, ACT_RELU, ACT_LRELU02 = 0, 1, 2
COLUMNS = ["fwd", "fwd_stats", "dgrad", "dgrad_stats", "wgrad", "wgrad_stats", "io0", "io1", "io2", "packed0", "packed1",
           "ws_fwd", "ws_dgrad", "ws_wgrad", "ws_dgrad_up2x", "head", "dgrad_act_fused"]


def geo(name, cin, h, w, cout, k, stride, pad, dil=1, aff0=False, act0=ACT_NONE, c1=0, act1=ACT_NONE, up2x=False):
    """One geometry: `cin` channels of the first source (+ `c1` of a second, which then carries an affine like the first)."""
    return dict(name=name, cin=cin, h=h, w=w, cout=cout, k=k, stride=stride, pad=pad, dil=dil, aff0=aff0, act0=act0, c1=c1,
                act1=act1, up2x=up2x)


def _unet7():
    g = []
    # down convs: k4 s2 p1; the previous level's BatchNorm + LeakyReLU ride in the gather (bn0 alone in front of the first)
    for i, (ci, co, h) in enumerate([(1, 64, 256), (64, 128, 128), (128, 256, 64), (256, 512, 32), (512, 512, 16), (512, 512, 8),
                                     (512, 512, 4)]):
        g.append(geo(f"unet7.down{i}", ci, h, h, co, 4, 2, 1, aff0=True, act0=ACT_LRELU02 if i else ACT_NONE))
    # up convs over the materialised relu + up2x + concat, innermost first
    for i, (ci, co, h) in enumerate([(1024, 512, 4), (1024, 512, 8), (1024, 512, 16), (1024, 256, 32), (512, 128, 64), (256, 64, 128)]):
        g.append(geo(f"unet7.up{i}", ci, h, h, co, 3, 1, 1))
    # the same levels with the upsample folded into the gather (two sources, each behind its BatchNorm + ReLU)
    for i, (c, co, h) in enumerate([(512, 512, 8), (512, 512, 16), (512, 256, 32), (256, 128, 64), (128, 64, 128)]):
        g.append(geo(f"unet7.up{i + 1}.fused", c, h, h, co, 3, 1, 1, aff0=True, act0=ACT_RELU, c1=c, act1=ACT_RELU, up2x=True))
    # the decoder head: two output channels over the virtual up2x(relu(affine(cat)))
    g.append(geo("unet7.head", 64, 256, 256, 2, 3, 1, 1, aff0=True, act0=ACT_RELU, c1=64, act1=ACT_RELU, up2x=True))
    g.append(geo("unet7.head.512x256", 64, 512, 256, 2, 3, 1, 1, aff0=True, act0=ACT_RELU, c1=64, act1=ACT_RELU, up2x=True))
    return g


GEOMETRIES = _unet7() + [
    geo("stem.7x7s2", 3, 224, 224, 64, 7, 2, 3),
    geo("stem.s2d.4x4", 16, 115, 115, 64, 4, 1, 0),
    geo("layer1.3x3@56", 64, 56, 56, 64, 3, 1, 1, aff0=True, act0=ACT_RELU),
    geo("layer1.3x3@56.plain", 64, 56, 56, 64, 3, 1, 1),
    geo("layer2.3x3s2", 64, 56, 56, 128, 3, 2, 1),
    geo("layer2.1x1s2", 64, 56, 56, 128, 1, 2, 0),
    geo("layer2.3x3@28", 128, 28, 28, 128, 3, 1, 1, aff0=True, act0=ACT_RELU),
    geo("layer3.3x3s2", 128, 28, 28, 256, 3, 2, 1),
    geo("layer3.1x1s2", 128, 28, 28, 256, 1, 2, 0),
    geo("layer3.3x3@14", 256, 14, 14, 256, 3, 1, 1, aff0=True, act0=ACT_RELU),
    geo("layer4.3x3@14", 256, 14, 14, 512, 3, 1, 1),
    geo("layer4.1x1s1", 256, 14, 14, 512, 1, 1, 0),
    geo("layer4.3x3@14.dil2", 512, 14, 14, 512, 3, 1, 2, dil=2, aff0=True, act0=ACT_RELU),
    geo("fc.512to32", 512, 14, 14, 32, 3, 1, 1),
    geo("map7x7", 512, 7, 7, 512, 3, 1, 1, aff0=True, act0=ACT_RELU),
    geo("ragged18x30", 64, 18, 30, 64, 3, 1, 1),
    geo("stft.1x4", 256, 1, 259, 1024, (1, 4), 1, 0),
    geo("smallco.plain", 8, 16, 16, 2, 3, 1, 1),
]
BATCHES = [1, 2, 8, 64]
PRECS = [0, 1]                       # AVSEP_PREC_F32, AVSEP_PREC_BF16
PLAN_NS = [0, 64]
ALGOS = [0, 1, 2, 4, 8, 16, 32, 64]  # none, then each single AVSEP_ALGO_NO_* bit (lib.ALGO_NO)
DUMMY = 256                          # a non-null address: the dispatch queries only check that it is set


def sweep():
    """Yields (label, ConvDesc) in the fixed order the stored index follows."""
    import avsep_amd as P
    assert sorted(P.lib.ALGO_NO.values()) == ALGOS[1:], "a new AVSEP_ALGO_NO_* bit: add it to ALGOS and regenerate on the parent"
    for g in GEOMETRIES:
        kh, kw = (g["k"], g["k"]) if isinstance(g["k"], int) else g["k"]
        for n in BATCHES:
            for prec in PRECS:
                for plan_n in PLAN_NS:
                    for algo in ALGOS:
                        d = P.lib.ConvDesc()
                        d.N, d.Cin, d.H, d.W, d.Cout = n, g["cin"] + g["c1"], g["h"], g["w"], g["cout"]
                        d.KH, d.KW, d.stride, d.pad, d.dil = kh, kw, g["stride"], g["pad"], g["dil"]
                        d.Ho = (g["h"] + 2 * g["pad"] - g["dil"] * (kh - 1) - 1) // g["stride"] + 1
                        d.Wo = (g["w"] + 2 * g["pad"] - g["dil"] * (kw - 1) - 1) // g["stride"] + 1
                        d.C0, d.act0, d.act1, d.up2x = g["cin"], g["act0"], g["act1"], int(g["up2x"])
                        d.prec, d.plan_n, d.algo = prec, plan_n, algo
                        d.x0 = DUMMY
                        if g["aff0"]:
                            d.scale0 = d.shift0 = DUMMY
                        if g["c1"]:
                            d.x1 = d.scale1 = d.shift1 = DUMMY
                        yield f"{g['name']} N={n} prec={prec} plan_n={plan_n} algo={algo}", d


def answers(L, d):
    """The answer row of one descriptor, in COLUMNS order."""
    ref = ctypes.byref(d)
    row = []
    buf = ctypes.create_string_buffer(128)
    for mode in (0, 1, 2):
        for with_stats in (0, 1):
            rc = L.avsep_conv_kernel_variant(ref, mode, with_stats, buf, len(buf))
            row.append(buf.value.decode() if rc == 0 else f"rc{rc}")
    for mode in (0, 1, 2):
        a, b = ctypes.c_int32(-1), ctypes.c_int32(-1)
        rc = L.avsep_conv_io_formats(ref, mode, ctypes.byref(a), ctypes.byref(b))
        row.append([rc, a.value, b.value])
    row += [L.avsep_conv_packed_floats(ref, 0), L.avsep_conv_packed_floats(ref, 1)]
    row += [L.avsep_conv2d_fwd_workspace_bytes(ref), L.avsep_conv2d_dgrad_workspace_bytes(ref),
            L.avsep_conv2d_wgrad_workspace_bytes(ref), L.avsep_conv2d_dgrad_up2x_workspace_bytes(ref)]
    row += [L.avsep_conv2d_head_applicable(ref), L.avsep_conv2d_dgrad_act_fused(ref)]
    return row


def build_table():
    """{"columns", "labels" (not stored), "rows": distinct answer rows, "index": row of each descriptor in sweep order}."""
    import avsep_amd as P
    L = P.lib.load()
    rows, where, index, labels = [], {}, [], []
    for label, d in sweep():
        r = answers(L, d)
        key = json.dumps(r)
        if key not in where:
            where[key] = len(rows)
            rows.append(r)
        index.append(where[key])
        labels.append(label)
    return {"columns": COLUMNS, "rows": rows, "index": index}, labels


def first_differences(stored, table, labels, limit=10):
    """[(label, column, stored answer, answer now)] of the first `limit` descriptors that answer differently."""
    out = []
    if stored["columns"] != table["columns"] or len(stored["index"]) != len(table["index"]):
        return [("the sweep itself", "columns / length", (stored["columns"], len(stored["index"])),
                 (table["columns"], len(table["index"])))]
    for label, i, j in zip(labels, stored["index"], table["index"]):
        a, b = stored["rows"][i], table["rows"][j]
        if a != b:
            out += [(label, c, x, y) for c, x, y in zip(COLUMNS, a, b) if x != y]
            if len(out) >= limit:
                break
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--table", default=TABLE)
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    table, labels = build_table()
    names = {r[c].split(":")[0] for r in table["rows"] for c in range(6)}
    print(f"{len(labels)} descriptors, {len(table['rows'])} distinct answer rows, {len(names)} kernel names: {sorted(names)}")
    if a.write:
        with open(a.table, "w") as f:
            f.write('{"columns": %s,\n "rows": [\n%s\n ],\n "index": %s}\n' % (
                json.dumps(table["columns"]), ",\n".join("  " + json.dumps(r) for r in table["rows"]),
                json.dumps(table["index"], separators=(",", ":"))))
        print(f"wrote {a.table} ({os.path.getsize(a.table)} bytes)")
        return 0
    with open(a.table) as f:
        stored = json.load(f)
    diffs = first_differences(stored, table, labels)
    for label, col, was, now in diffs:
        print(f"DIFF {label}: {col}: stored {was!r}, now {now!r}")
    print("no differences" if not diffs else f"{len(diffs)} differing answers shown")
    return 1 if diffs else 0


if __name__ == "__main__":
    sys.exit(main())
