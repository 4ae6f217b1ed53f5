"""gpu: evaluation visuals (csrc/visuals.hip, avsep_amd/visuals.py).  avsep_spec_image pixel by pixel against the float64
restatement in tests/visuals_ref.py under its derived gate (equality outside a band of 1e-3 level units around the integers,
either neighbour inside, at most 1 % of a case inside), item_images on the batch and outputs of one tiny forward under the
same gate, and the two switches end to end: train --mode eval --visuals and separate --report."""
import math
import os

import numpy as np
import pytest
import torch

import recipes
import visuals_ref as R
from test_visuals_host import parse_page

import avsep_amd as P
from avsep_amd import kernels as K
from avsep_amd import visuals as V
from avsep_amd import wavio

pytestmark = pytest.mark.gpu

TABLE = R.jet_table()


def check(got, v, rgb, what, exact=False):
    """The gate of visuals_ref.py: the share inside the band is printed before anything is asserted.  exact: the values are
    whole numbers by construction (a 0 / 1 mask times 255), where f32 is exact too: no band, the float64 floor everywhere."""
    got = got.cpu()
    exp, share = R.gate(got.numpy(), v, TABLE if rgb else None)
    if exact:
        assert np.array_equal(v, np.rint(v))
        exp, share = R.image(R.levels_of(v), TABLE if rgb else None), 0.0
    wrong = int((got != torch.from_numpy(exp)).any(-1).sum())
    print(f"{what}: {v.size} pixels, {100 * share:.3f} % inside the band, {wrong} wrong, "
          f"{100 * float((v > 255).mean()):.1f} % saturated")
    assert tuple(got.shape) == exp.shape and got.dtype == torch.uint8
    assert share <= R.SHARE, (what, share)
    assert torch.equal(got, torch.from_numpy(exp)), (what, wrong)


# shape, cell, reduce, mask (None | "soft" | a threshold), log, scale, rgb
CASES = [
    ((3, 5, 7), 1, "max", "soft", True, 200.0, True),        # T and W*3 no multiples of 4: scalar loads, byte stores
    ((3, 5, 7), 1, "max", None, True, 200.0, False),
    ((1, 1, 1), 1, "max", None, True, 200.0, True),
    ((1, 1, 1), 13, "mean", "soft", True, 200.0, False),     # cell > T: one column
    ((3, 5, 7), 2, "max", "soft", True, 200.0, True),        # cell does not divide T
    ((3, 5, 7), 3, "mean", 0.5, True, 200.0, True),
    ((3, 5, 7), 13, "max", None, True, 100.0, True),        # scale 100: the maxima of long cells do not all saturate
    ((3, 5, 7), 13, "mean", "soft", False, 10.0, False),
    ((2, 64, 96), 1, "max", "soft", True, 200.0, True),      # 16-byte loads, whole-dword stores
    ((2, 64, 96), 1, "max", None, True, 200.0, True),
    ((2, 64, 96), 1, "max", 0.5, True, 200.0, True),
    ((2, 64, 96), 1, "max", None, False, 100.0, True),       # the weight image's form
    ((2, 64, 96), 2, "max", 0.3, True, 200.0, True),
    ((2, 64, 96), 2, "mean", "soft", True, 200.0, False),
    ((2, 64, 96), 3, "mean", "soft", True, 200.0, True),
    ((2, 64, 96), 3, "max", None, False, 10.0, False),
    ((2, 64, 96), 13, "max", "soft", True, 100.0, True),     # 13 does not divide 96: a last cell of 5 frames
    ((2, 64, 96), 13, "mean", "soft", True, 200.0, True),
    ((2, 64, 98), 1, "max", "soft", True, 200.0, True),      # rows start on and off 16-byte boundaries in turn
    ((2, 64, 98), 2, "mean", 0.5, True, 200.0, True),        # W = 49: W*3 no multiple of 4
    ((2, 7, 1100), 3, "max", "soft", True, 200.0, True),     # W = 367: two passes of 256 columns per row
    ((2, 7, 1100), 32, "mean", "soft", True, 200.0, True),   # the longest staged cell
    ((2, 7, 1100), 33, "mean", "soft", True, 200.0, True),   # the shortest wave-per-column cell
    ((2, 7, 1100), 33, "max", 0.5, True, 100.0, False),
    ((2, 3, 5000), 40, "max", None, True, 100.0, True),      # W = 125: groups of four columns and a last group of one
    ((2, 3, 5000), 5003, "mean", "soft", True, 200.0, True),  # cell > T on the wave path
    ((2, 512, 256), 1, "max", "soft", True, 200.0, True),    # the reference's shape
    ((2, 512, 256), 1, "max", 0.5, True, 200.0, True),
    ((2, 512, 256), 1, "max", None, False, 100.0, True),
    ((3, 512, 5000), 3, "max", "soft", True, 200.0, True),   # the strip form: W = 1667, many blocks, strided work
    ((3, 512, 5000), 3, "mean", None, False, 255.0, False),  # its mask picture
]


def _id(c):
    shape, cell, red, mask, log, scale, rgb = c
    return f"{'x'.join(map(str, shape))}-c{cell}-{red}-{mask}-{'log' if log else 'lin'}{int(scale)}-{'rgb' if rgb else 'grey'}"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_spec_image_against_the_restatement(dev, case):
    shape, cell, red, mask, log, scale, rgb = case
    mag, msk = R.draw(shape, 0)
    if not log and scale == 255.0:                           # the grey mask form: the mask itself is the picture
        mag = msk
    m = None if mask is None else msk
    thres = mask if isinstance(mask, float) else None
    v = R.values(mag, m, thres, cell, red, log, scale)
    got = K.spec_image(torch.from_numpy(mag).to(dev), None if m is None else torch.from_numpy(m).to(dev), thres, cell, red,
                       log, scale, torch.from_numpy(TABLE).to(dev) if rgb else None)
    check(got, v, rgb, _id(case))
    if shape == (2, 64, 96) and cell == 1 and mask == "soft":          # a second call gives the same bytes
        again = K.spec_image(torch.from_numpy(mag).to(dev), torch.from_numpy(m).to(dev), thres, cell, red, log, scale,
                             torch.from_numpy(TABLE).to(dev) if rgb else None)
        assert torch.equal(got, again)


def test_grey_mask_form_is_clip_times_255(dev):
    """log 0, scale 255, no table on a mask with values outside [0, 1]: clip(mask, 0, 1) * 255 truncated (main.py:375-376),
    under the gate; exact zeros, ones, negatives and a NaN included."""
    rng = np.random.default_rng(5)
    m = rng.uniform(-0.3, 1.3, (2, 33, 50)).astype(np.float32)
    m[0, 0, :4] = [0.0, 1.0, -0.0, np.nan]
    got = K.spec_image(torch.from_numpy(m).to(dev), log=False, scale=255.0)
    check(got, R.values(m, log=False, scale=255.0), False, "grey mask")
    g = got.cpu().numpy()[..., 0][:, ::-1]                               # back in source row order
    assert g[0, 0, :4].tolist() == [0, 255, 0, 0]
    assert np.all(g[m < 0] == 0) and np.all(g[m >= 1] == 255)


def test_special_values_by_hand(dev):
    """Saturation, negative values, infinities and NaN on every path of the kernel (cell 1, staged, wave per column)."""
    row = np.array([0.0, 9.05, 17.0, 18.0, 1e30, np.inf, -0.5, -2.0, -np.inf, np.nan, 3.0, 0.5], dtype=np.float32)
    want = [0, 200, 251, 255, 255, 255, 0, 0, 0, 0, 120, 35]
    got = K.spec_image(torch.from_numpy(row.reshape(1, 1, -1)).to(dev))
    assert got[0, 0, :, 0].tolist() == want == R.spec_image(row.reshape(1, 1, -1))[0, 0, :, 0].tolist()
    for cell in (2, 40):                                                 # a NaN in a cell stays under max and under mean
        x = np.ones((1, 2, 3 * cell), dtype=np.float32)
        x[0, 0, cell + 1] = np.nan
        x[0, 1, 0] = np.inf
        for red in ("max", "mean"):
            got = K.spec_image(torch.from_numpy(x).to(dev), cell=cell, reduce=red, log=False, scale=100.0)
            assert got[..., 0].tolist() == [[[255, 100, 100], [100, 0, 100]]] == \
                R.spec_image(x, cell=cell, reduce=red, log=False, scale=100.0)[..., 0].tolist(), (cell, red)


@pytest.mark.parametrize("rgb", [True, False], ids=["rgb", "grey"])
@pytest.mark.parametrize("cell", [1, 3, 40])
def test_output_one_byte_into_its_buffer(dev, rgb, cell):
    """An output that starts one byte past a 4-byte boundary: no store may be a whole dword unless its address allows it, and
    the guard bytes before and after the image keep their value."""
    shape = (2, 9, 96 * cell)
    mag, msk = R.draw(shape, 3)
    ch, W = (3 if rgb else 1), 96
    n = shape[0] * shape[1] * W * ch
    buf = torch.full((n + 16,), 0xA5, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 4 == 0
    out = buf[1:1 + n].view(shape[0], shape[1], W, ch)
    table = torch.from_numpy(TABLE).to(dev) if rgb else None
    got = K.spec_image(torch.from_numpy(mag).to(dev), torch.from_numpy(msk).to(dev), None, cell, "max", True, 200.0, table, out=out)
    assert got.data_ptr() == buf.data_ptr() + 1
    check(got, R.values(mag, msk, None, cell, "max"), rgb, f"offset output, cell {cell}")
    assert buf[0].item() == 0xA5 and bool((buf[1 + n:] == 0xA5).all())
    aligned = K.spec_image(torch.from_numpy(mag).to(dev), torch.from_numpy(msk).to(dev), None, cell, "max", True, 200.0, table)
    assert torch.equal(aligned, got)                                     # the byte path and the dword path agree


def test_input_views_off_a_16_byte_boundary(dev):
    """Magnitudes and masks that start 4 bytes past a 16-byte boundary take the scalar loads and give the same picture."""
    shape = (2, 5, 64)
    mag, msk = R.draw(shape, 4)
    n = mag.size
    bm, bk = (torch.zeros(n + 4, device=dev) for _ in range(2))
    bm[1:1 + n] = torch.from_numpy(mag).reshape(-1).to(dev)
    bk[1:1 + n] = torch.from_numpy(msk).reshape(-1).to(dev)
    for cell in (1, 2):
        got = K.spec_image(bm[1:1 + n].view(shape), bk[1:1 + n].view(shape), None, cell)
        check(got, R.values(mag, msk, None, cell), False, f"offset input, cell {cell}")


def test_strided_operands_are_densified_for_the_launch(dev):
    """Magnitude AND mask as strided views (transposes of [F,R,T] buffers): the wrapper's two dense copies are of equal size,
    and both must be alive when the kernel runs.  The picture is that of the dense operands, under the gate."""
    shape = (6, 40, 96)
    mag, msk = R.draw(shape, 6)
    table = torch.from_numpy(TABLE).to(dev)
    tm = torch.from_numpy(np.ascontiguousarray(mag.transpose(1, 0, 2))).to(dev).transpose(0, 1)
    tk = torch.from_numpy(np.ascontiguousarray(msk.transpose(1, 0, 2))).to(dev).transpose(0, 1)
    assert not tm.is_contiguous() and not tk.is_contiguous() and tuple(tm.shape) == shape
    for cell, red in ((1, "max"), (3, "mean")):
        got = K.spec_image(tm, tk, None, cell, red, table=table)
        check(got, R.values(mag, msk, None, cell, red), True, f"strided operands, cell {cell}")
        assert torch.equal(got, K.spec_image(tm.contiguous(), tk.contiguous(), None, cell, red, table=table))
    got = K.spec_image(tm, None, None, 1, table=table)                     # the magnitude alone strided
    check(got, R.values(mag), True, "strided magnitude")
    got = K.spec_image(torch.from_numpy(mag).to(dev), tk, 0.5, 1, table=table)
    check(got, R.values(mag, msk, 0.5), True, "strided mask")


def test_launcher_refusals(dev):
    """avsep_spec_image itself: null pointers, non-positive sizes, cell < 1, reduce or log outside {0, 1} and a row count
    beyond one launch are AVSEP_ERR_ARG, and the output keeps its bytes."""
    L = P.lib.load()
    mag = torch.ones(2, 3, 4, device=dev)
    out = torch.full((2, 3, 4, 1), 7, dtype=torch.uint8, device=dev)
    nan = float("nan")

    def run(mag_p=mag.data_ptr(), R_=2, F=3, T=4, cell=1, red=0, log=1, out_p=out.data_ptr()):
        return L.avsep_spec_image(mag_p, None, nan, R_, F, T, cell, red, log, 200.0, None, out_p, P.lib.stream())
    bad = [dict(mag_p=None), dict(out_p=None), dict(R_=0), dict(F=0), dict(T=0), dict(R_=-1), dict(T=-4), dict(cell=0), dict(cell=-1),
           dict(red=2), dict(red=-1), dict(log=2), dict(log=-1), dict(R_=65536, F=32768)]
    for kw in bad:
        assert run(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool((out == 7).all())
    assert run() == 0
    torch.cuda.synchronize()
    assert out.flatten().tolist() == [60] * 24                            # log10(2) * 200 = 60.2


# ---------------------------------------------------------------------------------------------------------------------
# item_images on one tiny forward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_vis", [True, False], ids=["av", "ao"])
def test_item_images_against_the_restatement(dev, use_vis):
    (snd, frm), gen = recipes.small_nets(dev, 7)
    mb = P.ModelBuilder()
    wrap = P.NetWrapper((snd, frm), mb.build_criterion("bce", use_pit=True), mb.build_criterion("bce"))
    wrap.eval()
    args = recipes.args(weighted_loss=1, match_weight=0.1, stft_frame=128, stft_hop=32, mask_thres=0.5)
    B, Fin, T = 2, 65, 64
    srcs = [torch.rand(B, 1, Fin, T, generator=gen) ** 2 * 4 for _ in range(2)]
    batch = {"mag_mix": (srcs[0] + srcs[1]).to(dev), "mags": [s.to(dev) for s in srcs],
             "frames": [torch.randn(B, 3, 2, 64, 64, generator=gen).to(dev) for _ in range(2)]}
    with torch.no_grad():
        _, outputs = wrap.forward(batch, args, use_vis)
        before = {k: [t.clone() for t in outputs[k]] for k in ("pred_masks", "gt_masks")}
        images = V.item_images(batch, outputs, args)
        first = V.item_images(batch, outputs, args, items=1)
        # the linear masks, independently of visuals.py: kernels.warp's un-warp of every mask, source by source
        unwarp = lambda m: K.warp(m.detach().float().contiguous(), Fin, T, 0)[:, 0]                 # noqa: E731
        pred_lin = torch.stack([unwarp(m) for m in outputs["pred_masks"]], 0)
        gt_lin = torch.stack([unwarp(m) for m in outputs["gt_masks"]], 0)
        lin_v = V.linear_masks(outputs, args, Fin)
    assert all(torch.equal(a, b) for k in before for a, b in zip(before[k], outputs[k]))             # nothing was changed
    assert sorted(images) == sorted(["mix", "weight"] + [f"{k}{n}" for k in ("predamp", "gtamp", "predmask", "gtmask") for n in (1, 2)])
    cpu = lambda t: t.detach().float().cpu().numpy()                     # noqa: E731
    mag = cpu(batch["mag_mix"])[:, 0]
    weight = cpu(outputs["weight"])
    weight = weight[:, 0] if use_vis else weight[..., 0]
    assert images["mix"].shape == (B, 256, T, 3) and images["predamp1"].shape == (B, Fin, T, 3)
    assert images["predmask2"].shape == (B, 256, T)
    check(images["mix"], R.values(cpu(outputs["mag_mix"])[:, 0]), True, "mix")
    check(images["weight"], R.values(weight, log=False, scale=100.0), True, "weight")
    assert torch.equal(lin_v[0], pred_lin.reshape(2 * B, Fin, T)) and torch.equal(lin_v[1], gt_lin.reshape(2 * B, Fin, T))
    assert sorted(first) == sorted(images) and all(torch.equal(first[k], images[k][:1]) for k in images)     # items=1: the first item
    pred_lin, gt_lin = cpu(pred_lin), cpu(gt_lin)
    assert not np.array_equal(gt_lin[0], gt_lin[1]) and not np.array_equal(pred_lin[0], pred_lin[1])     # a swap would show
    for n in range(2):
        check(images[f"predamp{n + 1}"], R.values(mag, pred_lin[n], args.mask_thres), True, f"predamp{n + 1}")
        check(images[f"gtamp{n + 1}"], R.values(mag, gt_lin[n]), True, f"gtamp{n + 1}")
        pm = (cpu(outputs["pred_masks"][n])[:, 0] > np.float32(args.mask_thres)).astype(np.float32)
        check(images[f"predmask{n + 1}"][..., None], R.values(pm, log=False, scale=255.0), False, f"predmask{n + 1}", exact=True)
        check(images[f"gtmask{n + 1}"][..., None], R.values(cpu(outputs["gt_masks"][n])[:, 0], log=False, scale=255.0), False,
              f"gtmask{n + 1}", exact=True)                                  # binary_mask 1: the true masks are 0 / 1 as well
    assert set(np.unique(images["predmask1"].cpu().numpy()).tolist()) <= {0, 255}


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
def _srcs_exist(index):
    page = parse_page(index)
    root = os.path.dirname(index)
    assert page.src and all(os.path.isfile(os.path.join(root, s)) for s in page.src), page.src
    return page


def test_eval_mode_writes_the_visuals(dev, tmp_path, capsys):
    from PIL import Image
    from avsep_amd import train as T
    from test_dataset import _make_disk_dataset
    full = _make_disk_dataset(str(tmp_path))
    with open(full) as f:
        two = f.read().splitlines()[:2]
    lst = str(tmp_path / "two.csv")
    with open(lst, "w") as f:
        f.write("\n".join(two) + "\n")
    ck = tmp_path / "ck" / "run"
    os.makedirs(str(ck))
    mb = P.ModelBuilder()
    torch.manual_seed(11)
    torch.save(mb.build_sound(arch="unet5", fc_dim=2, fusion_type="hidsep", att_type="sig").state_dict(), str(ck / "sound_best.pth"))
    torch.save(mb.build_frame(arch="resnet18dilated", fc_dim=256, pool_type="maxpool").state_dict(), str(ck / "frame_best.pth"))
    flags = ("--id run --ckpt {ck} --av_list_train {l} --ao_list_train {l} --list_val {l} --mode eval "
             "--arch_sound unet5 --arch_frame resnet18dilated --img_pool maxpool --num_channels 2 --img_activation relu "
             "--output_activation sigmoid --vis_channels 256 --fusion_type hidsep --not_pool_vis --att_type sig "
             "--binary_mask 1 --loss bce --weighted_loss 1 --num_mix 2 --log_freq 1 --num_frames 2 --stride_frames 2 "
             "--imgSize 64 --audLen 65535 --margin 1.0 --batch_size_per_gpu 2 --workers 0 --val_repeat 1 "
             "--rate_dc 0 --rate_sc 1 --max_silent 0.87").format(ck=str(tmp_path / "ck"), l=lst).split()
    import shutil
    shutil.copytree(str(ck), str(tmp_path / "ck" / "one"))                # the same weights under a second --id
    summary = lambda text: [l for l in text.splitlines() if l.startswith("[Eval Summary]")]         # noqa: E731
    capsys.readouterr()
    T.cli(flags)
    plain = summary(capsys.readouterr().out)
    assert len(plain) == 2 and not os.path.exists(str(ck / "visualization"))
    T.cli(flags + ["--visuals", "--num_vis", "2"])
    out = capsys.readouterr().out
    assert summary(out) == plain, (summary(out), plain)                   # the printed metrics do not move
    a = P.ArgParser().parse_train_arguments(flags, verbose=False)
    for mode in ("av", "ao"):
        root = str(ck / "visualization" / mode)
        page = _srcs_exist(os.path.join(root, "index.html"))
        assert page.th == len(V.page_header(2)) and page.tr == 1 + 2
        items = sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d)))
        assert len(items) == 2
        item = os.path.join(root, items[0])
        assert sorted(os.listdir(item)) == sorted(
            ["mix.jpg", "mix.wav", "weight.jpg"] + [f"{k}{n}.{e}" for n in (1, 2) for k, e in (
                ("predamp", "jpg"), ("gtamp", "jpg"), ("predmask", "jpg"), ("gtmask", "jpg"), ("pred", "wav"), ("gt", "wav"),
                ("frames", "png"))])
        with Image.open(os.path.join(item, "mix.jpg")) as im:
            assert im.size == (256, 256) and im.mode == "RGB"
        with Image.open(os.path.join(item, "predamp1.jpg")) as im:
            assert im.size == (256, a.stft_frame // 2 + 1) and im.mode == "RGB"
        with Image.open(os.path.join(item, "predmask1.jpg")) as im:
            assert im.size == (256, 256) and im.mode == "L"
        with Image.open(os.path.join(item, "frames1.png")) as im:
            assert im.size == (2 * 64, 64) and im.mode == "RGB"
        info = wavio.probe(os.path.join(item, "pred1.wav"))
        # pred_wavs are the iSTFT of 1 + audLen // hop frames: hop * (frames - 1) samples
        assert info.fmt == "s24" and info.rate == a.audRate and info.channels == 1
        assert info.frames == a.stft_hop * (a.audLen // a.stft_hop)
        raw, _ = wavio.read_frames(os.path.join(item, "gt2.wav"))
        assert np.abs(wavio.decode(raw, "s24", 1)).max() <= 1.0
    # --num_vis 1 stops after the first item of the batch
    T.cli(["one" if f == "run" else f for f in flags] + ["--visuals", "--num_vis", "1"])
    for mode in ("av", "ao"):
        root = str(tmp_path / "ck" / "one" / "visualization" / mode)
        assert _srcs_exist(os.path.join(root, "index.html")).tr == 2
        assert len([d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d))]) == 1


def test_separate_report(dev, tmp_path):
    from PIL import Image
    from avsep_amd import separate as S
    mb = P.ModelBuilder()
    torch.manual_seed(11)
    torch.save(mb.build_sound(arch="unet5", fc_dim=2, fusion_type="hidsep", att_type="sig").state_dict(), str(tmp_path / "sound.pth"))
    torch.save(mb.build_frame(arch="resnet18dilated", fc_dim=256, pool_type="maxpool").state_dict(), str(tmp_path / "frame.pth"))
    rate = 11025
    pcm = recipes.tone_mix_stereo(8 * rate, rate, 8)
    recipes.write_pcm(str(tmp_path / "mix.wav"), pcm, rate)
    argv = ["--wav", str(tmp_path / "mix.wav"), "--audio_only", "--arch_sound", "unet5", "--num_channels", "2", "--vis_channels", "256",
            "--img_pool", "maxpool", "--not_pool_vis", "--fusion_type", "hidsep", "--att_type", "sig", "--weights_sound",
            str(tmp_path / "sound.pth"), "--weights_frame", str(tmp_path / "frame.pth"), "--binary_mask", "0", "--channels", "keep"]
    S.cli(argv + ["--out", str(tmp_path / "plain")])
    S.cli(argv + ["--out", str(tmp_path / "rep"), "--report", "--report_width", "100"])
    assert sorted(os.listdir(str(tmp_path / "plain"))) == ["source0.wav", "source1.wav"]
    assert sorted(os.listdir(str(tmp_path / "rep"))) == ["mask0.png", "mask1.png", "mix.png", "report.html", "source0.png",
                                                         "source0.wav", "source1.png", "source1.wav"]
    for n in range(2):                                                    # the stems are bit for bit those of the plain run
        assert recipes.file_bytes(tmp_path / "plain" / f"source{n}.wav") == recipes.file_bytes(tmp_path / "rep" / f"source{n}.wav")
    a = S.parse_args(argv)
    frames = 1 + (8 * rate) // a.stft_hop
    cell = math.ceil(frames / 100)
    assert cell == 4 and V.report_cell(frames, 100) == cell
    W, Fin = math.ceil(frames / cell), a.stft_frame // 2 + 1
    for name, mode in (("mix.png", "RGB"), ("source0.png", "RGB"), ("source1.png", "RGB"), ("mask0.png", "L"), ("mask1.png", "L")):
        with Image.open(str(tmp_path / "rep" / name)) as im:
            assert im.size == (W, Fin) and im.mode == mode, name
    page = _srcs_exist(str(tmp_path / "rep" / "report.html"))
    assert page.tr == 2 and page.th == 2 + 2 * 2
    assert "before any Wiener filter or phase iteration" in " ".join(page.text)
    # mix.png is the kernel's picture of the down-mix's STFT, low frequencies at the bottom
    wav = torch.from_numpy(pcm.astype(np.float32).mean(1) / 32768.0).to(dev)
    mag = K.Stft(dev, a.stft_frame, a.stft_hop).stft(wav[None], want_phase=False)[0]
    with Image.open(str(tmp_path / "rep" / "mix.png")) as im:
        got = torch.from_numpy(np.array(im))[None]
    check(got, R.values(mag.cpu().numpy(), cell=cell), True, "report mix.png")


def test_report_pictures_take_the_threshold_of_binary_stems(dev, tmp_path):
    """separate's default is --binary_mask 1: a stem is mag * (M > mask_thres) (mask_stitch), so its picture takes the same
    threshold inside the kernel, the mask picture stays the blended mask, and the page says so."""
    import argparse
    from PIL import Image
    rate, hop = 11025, 256
    wav = recipes.tone_mix(3 * rate, 5).to(dev)
    a = argparse.Namespace(stft_frame=1022, stft_hop=hop, audRate=rate, binary_mask=1, mask_thres=0.5)
    mag = K.Stft(dev, a.stft_frame, hop).stft(wav[None], want_phase=False)[0][0].contiguous()
    Fin, F = mag.shape
    lin = torch.rand((2, Fin, F), generator=torch.Generator().manual_seed(2)).to(dev)
    cell = V.report(str(tmp_path / "bin"), wav, lin, a, width=50)
    assert cell == math.ceil(F / 50) == 3
    magn, linn = mag.cpu().numpy(), lin.cpu().numpy()
    for n in range(2):
        with Image.open(str(tmp_path / "bin" / f"source{n}.png")) as im:
            check(torch.from_numpy(np.array(im))[None], R.values(magn[None], linn[n:n + 1], 0.5, cell), True, f"binary source{n}.png")
        with Image.open(str(tmp_path / "bin" / f"mask{n}.png")) as im:
            check(torch.from_numpy(np.array(im))[None, ..., None], R.values(linn[n:n + 1], None, None, cell, "mean", False, 255.0),
                  False, f"mask{n}.png")
    assert "thresholded at 0.5" in " ".join(parse_page(str(tmp_path / "bin" / "report.html")).text)
    a.binary_mask = 0
    V.report(str(tmp_path / "soft"), wav, lin, a, width=50)
    with Image.open(str(tmp_path / "soft" / "source0.png")) as im:
        check(torch.from_numpy(np.array(im))[None], R.values(magn[None], linn[:1], None, cell), True, "soft source0.png")
    assert "thresholded" not in " ".join(parse_page(str(tmp_path / "soft" / "report.html")).text)
