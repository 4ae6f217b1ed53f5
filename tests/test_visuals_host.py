"""not-gpu: the float64 restatement of the image rule (tests/visuals_ref.py) against hand-made cases, the argument refusals
of kernels.spec_image, the page writer and the --visuals / --report switches."""
import os
from html.parser import HTMLParser

import numpy as np
import pytest
import torch

import recipes
import visuals_ref as R

from avsep_amd import kernels as K
from avsep_amd import visuals as V
from avsep_amd.lib import AvsepError


# ---- the restatement ---------------------------------------------------------------------------------------------------
def _one(v, **kw):
    return R.spec_image(np.array(v, dtype=np.float32).reshape(1, 1, -1), **kw)[0, 0, :, 0].tolist()


def test_zero_saturation_negative_and_nan():
    assert _one([0.0]) == [0]                                            # log10(1) * 200
    assert _one([9.0]) == [200] and _one([17.0]) == [251]                # log10(10) * 200; log10(18) * 200 = 251.05
    assert _one([18.0, 1e6, np.inf]) == [255, 255, 255]                  # 255.75 and beyond: saturated, not wrapped
    assert _one([-0.5, -2.0, np.nan]) == [0, 0, 0]                       # log10(0.5) < 0; log10(-1) and NaN are NaN
    assert _one([2.549, 2.55, 2.56, -1.0], log=False, scale=100.0) == [254, 254, 255, 0]     # f32(2.55) * 100 < 255
    assert _one([np.nan], log=False, scale=100.0) == [0]


def test_row_flip_and_table():
    mag = np.zeros((2, 3, 1), dtype=np.float32)
    mag[0, 0, 0], mag[1, 2, 0] = 9.0, 99.0                               # levels 200 and (saturated) 255
    grey = R.spec_image(mag)
    assert grey.shape == (2, 3, 1, 1)
    assert grey[0, :, 0, 0].tolist() == [0, 0, 200] and grey[1, :, 0, 0].tolist() == [255, 0, 0]
    table = R.jet_table()
    rgb = R.spec_image(mag, table=table)
    assert rgb.shape == (2, 3, 1, 3) and rgb[0, 2, 0].tolist() == table[200].tolist() and rgb[0, 0, 0].tolist() == table[0].tolist()
    assert table[0].tolist() == [0, 0, 128] and table[255].tolist() == [131, 0, 0] and table[128].tolist() == [128, 255, 128]
    from avsep_amd.localise import jet_table
    assert np.array_equal(table, jet_table())


def test_cells_partial_last_cell_and_one_column():
    row = [1.0, 3.0, 2.0, 0.0, 4.0]                                      # cells of 2: (1,3) (2,0) (4)
    assert _one(row, cell=2, log=False, scale=10.0) == [30, 20, 40]
    assert _one(row, cell=2, reduce="mean", log=False, scale=10.0) == [20, 10, 40]          # the last mean is over ONE frame
    assert _one(row, cell=3, reduce="mean", log=False, scale=10.0) == [20, 20]
    assert _one(row, cell=13, log=False, scale=10.0) == [40]                                # cell > T: one column
    assert _one(row, cell=13, reduce="mean", log=False, scale=10.0) == [20]
    assert R.values(np.zeros((2, 3, 5), np.float32), cell=2).shape == (2, 3, 3)


def test_mask_threshold_and_grey_form():
    mag = np.array([4.0, 4.0, 4.0], dtype=np.float32).reshape(1, 1, 3)
    mask = np.array([0.25, 0.5, 0.75], dtype=np.float32).reshape(1, 1, 3)
    assert R.spec_image(mag, mask, log=False, scale=10.0)[0, 0, :, 0].tolist() == [10, 20, 30]
    assert R.spec_image(mag, mask, 0.5, log=False, scale=10.0)[0, 0, :, 0].tolist() == [0, 0, 40]     # > thres, not >=
    m = np.array([-0.2, 0.0, 0.3, 0.999, 1.0, 1.7], dtype=np.float32).reshape(1, 1, 6)
    grey = R.spec_image(m, log=False, scale=255.0)[0, 0, :, 0]
    assert np.array_equal(grey, (np.clip(m[0, 0], 0, 1) * 255).astype(np.uint8))             # main.py:375-376
    # the product is the f32 product: 0.1f * 3f = 0.3f + 1 ulp in f32, 0.30000000447 in float64
    v = R.values(np.float32([[[0.1]]]), np.float32([[[3.0]]]), log=False, scale=1.0)
    assert v[0, 0, 0] == float(np.float32(0.1) * np.float32(3.0))


def test_gate_accepts_a_neighbour_only_inside_the_band():
    v = np.array([[[10.5, 11.0004, 11.9995, 255.0003]]])
    exact = R.levels_of(v)[..., None]
    assert exact[0, 0, :, 0].tolist() == [10, 11, 11, 255]
    exp, share = R.gate(exact, v)
    assert np.array_equal(exp, exact) and share == 0.75
    other = exact.copy()
    other[0, 0, :, 0] = [11, 10, 12, 254]                                # the first is outside the band: still refused
    exp, _ = R.gate(other, v)
    assert exp[0, 0, :, 0].tolist() == [10, 10, 12, 254]
    far = exact.copy()
    far[0, 0, 1, 0] = 13                                                 # inside the band, but no neighbour
    assert R.gate(far, v)[0][0, 0, 1, 0] == 11


def test_the_draw_exercises_band_and_clamp():
    """The figures the GPU gate relies on, at the issue's shape and seed: well under 1 % of the pixels lie inside the band
    and some saturate."""
    mag, mask = R.draw((4, 64, 96), 0)
    for kw in (dict(mask=mask), dict(), dict(mask=None, log=False, scale=255.0)):
        src = mask if "log" in kw else mag
        v = R.values(src, kw.get("mask"), log=kw.get("log", True), scale=kw.get("scale", 200.0))
        _, share = R.gate(R.levels_of(v)[..., None], v)
        assert 0.0005 < share < 0.006, share
    assert 0.01 < (R.values(mag, mask) > 255).mean() < 0.06 and 0.10 < (R.values(mag) > 255).mean() < 0.20


# ---- kernels.spec_image refuses before it launches ---------------------------------------------------------------------
def test_spec_image_refusals(monkeypatch):
    recipes.no_gpu_call(monkeypatch)
    mag = torch.zeros(2, 4, 6)
    table = torch.zeros(256, 3, dtype=torch.uint8)
    bad = [dict(mag=mag.double()), dict(mag=mag[0]), dict(mag=torch.zeros(0, 4, 6)), dict(mag=np.zeros((2, 4, 6), np.float32)),
           dict(mask=torch.zeros(2, 4, 5)), dict(mask=mag.double()), dict(thres=0.5), dict(mask=mag, thres=float("nan")),
           dict(cell=0), dict(cell=-3), dict(cell=2.0), dict(cell=True), dict(reduce="sum"), dict(reduce=1),
           dict(scale=float("nan")), dict(table=torch.zeros(256, 3)), dict(table=torch.zeros(255, 3, dtype=torch.uint8)),
           dict(out=torch.zeros(2, 4, 6, 3, dtype=torch.uint8)), dict(table=table, out=torch.zeros(2, 4, 6, 1, dtype=torch.uint8)),
           dict(cell=4, out=torch.zeros(2, 4, 6, 1, dtype=torch.uint8)), dict(out=torch.zeros(2, 4, 6, 1))]
    for kw in bad:
        with pytest.raises(AvsepError):
            K.spec_image(**{"mag": mag, **kw})
    with pytest.raises(AvsepError, match="no CPU fallback"):             # everything in order, but not on a GPU
        monkeypatch.undo()
        K.spec_image(mag)
    with pytest.raises(AvsepError):
        V.report_cell(100, 0)
    assert V.report_cell(25840, 2048) == 13 and V.report_cell(100, 2048) == 1 and V.report_cell(2049, 2048) == 2


# ---- the page ----------------------------------------------------------------------------------------------------------
class _Page(HTMLParser):
    def __init__(self):
        super().__init__()
        self.src, self.th, self.tr, self.td, self.tags, self.text = [], 0, 0, 0, [], []

    def handle_starttag(self, tag, attrs):
        self.tags.append(tag)
        self.th += tag == "th"
        self.tr += tag == "tr"
        self.td += tag == "td"
        self.src += [v for k, v in attrs if k == "src"]

    def handle_data(self, data):
        self.text.append(data)


def parse_page(path):
    p = _Page()
    with open(path, encoding="utf-8") as f:
        p.feed(f.read())
    return p


def test_page_writer(tmp_path):
    names = ["a b/mix.jpg", "a b/mix.wav", "x&y/p\"1.jpg"]
    for n in names:
        os.makedirs(os.path.dirname(str(tmp_path / n)), exist_ok=True)
        (tmp_path / n).write_bytes(b"x")
    nasty = "<script>alert('1')</script> & \"co\""
    rows = [[{"text": [nasty, "SDR: 1.00, -2.00"]}, {"image": names[0], "audio": names[1]}, {"image": names[2]}],
            [{"text": "second"}, {"image": names[0]}, {"text": "audio only"}]]
    V.write_page(str(tmp_path / "index.html"), ["item <1>", "mixture", "mask & more"], rows, note="a <note>")
    raw = (tmp_path / "index.html").read_text(encoding="utf-8")
    assert "<script>" not in raw and "&lt;script&gt;" in raw and "item &lt;1&gt;" in raw and "a &lt;note&gt;" in raw
    assert "p&quot;1.jpg" in raw and "x&amp;y" in raw
    page = parse_page(str(tmp_path / "index.html"))
    assert page.th == 3 and page.tr == 1 + len(rows) and page.td == 6
    assert "script" not in page.tags and page.tags.count("img") == 3 and page.tags.count("audio") == 1
    assert sorted(page.src) == sorted([names[0], names[1], names[2], names[0]])
    assert all(os.path.exists(str(tmp_path / s)) for s in page.src)
    assert nasty in page.text                                             # what a browser shows is the text itself
    assert len(V.page_header(2)) == 2 + 5 * 2 + 1 and len(V.page_header(3)) == 18
    assert V._folder("a/b") == "a-b" and V._folder("..") == "item" and V._folder("") == "item"


def test_frame_strips_round_and_clamp():
    mean, std = torch.tensor(V.MEAN).view(3, 1, 1), torch.tensor(V.STD).view(3, 1, 1)
    u8 = torch.tensor([0, 1, 127, 254, 255], dtype=torch.float32).view(1, 1, 5).expand(3, 2, 5)      # [3,H=2,W=5]
    one = (u8 / 255.0 - mean) / std
    frames = torch.stack([one, one.flip(-1), one * 4.0], 1)[None]          # [1,3,T=3,2,5]; the third overshoots both ways
    strip = V.frame_strips(frames)
    assert strip.shape == (1, 2, 15, 3) and strip.dtype == torch.uint8
    assert strip[0, 0, :5, 1].tolist() == [0, 1, 127, 254, 255] and strip[0, 1, 5:10, 2].tolist() == [255, 254, 127, 1, 0]
    assert int(strip[0, 0, 10:, 0].min()) == 0 and int(strip[0, 0, 10:, 0].max()) == 255


# ---- the switches ------------------------------------------------------------------------------------------------------
def test_own_flags_and_report_flags():
    from avsep_amd import separate as S
    from avsep_amd import train as T
    own, rest = T.own_flags(["--id", "x", "--visuals", "--num_vis", "3"])
    assert own.visuals is True and own.gpu_frames is False and rest == ["--id", "x", "--num_vis", "3"]
    own, rest = T.own_flags(["--gpu_frames"])
    assert own.visuals is False and own.gpu_frames is True and rest == []
    assert "no HTML visualisation" not in T.__doc__ and "--visuals" in T.__doc__
    a = S.parse_args(["--wav", "x.wav", "--audio_only"])
    assert a.report is False and a.report_width == 2048
    a = S.parse_args(["--wav", "x.wav", "--audio_only", "--report", "--report_width", "640"])
    assert a.report is True and a.report_width == 640
    with pytest.raises(SystemExit):
        S.parse_args(["--wav", "x.wav", "--audio_only", "--report", "--report_width", "0"])
