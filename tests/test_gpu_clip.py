"""gpu: separating with a clip (avsep_window_reduce in csrc/longform.hip, separate_long(frame_times=..., return_maps=...), the
duet form, the command line) against the NumPy float32 loop of tests/clip_ref.py, float64 means and the oracle nets on the
CPU — never the code under test.  Helpers of test_gpu_longform.py are imported, not copied."""
import types

import numpy as np
import pytest
import torch

from conftest import assert_close, rel_err

import avsep_amd as P
from avsep_amd import separate as S
from oracle import inference as OI

import clip_ref as R
from recipes import args as _args, tone_mix as _tone_mix
import test_gpu_longform as LF

pytestmark = pytest.mark.gpu

RATE, HOP = 11025, 256


# ---------------------------------------------------------------------------------------------------------------------
# kernel
# ---------------------------------------------------------------------------------------------------------------------
def _tables(T):
    """The (first, count) tables of one T: K = 1 (the whole range) and K = 70 (single frames, the whole range, overlapping
    consecutive ranges, two identical rows, rows ending at T - 1)."""
    rows = [(0, T), (T - 1, 1), (0, 1), (0, T)]                                  # whole range twice: identical rows
    step = 0
    while len(rows) < 70:                                                       # overlapping consecutive ranges, cyclically
        first = (2 * step) % T
        rows.append((first, min(4 + step % 3, T - first)))
        step += 1
    rows[-1] = (T // 2, T - T // 2)                                             # ends at T - 1
    assert len(rows) == 70 and any(c == 1 for _, c in rows) and all(c >= 1 and 0 <= f and f + c <= T for f, c in rows)
    return {"K=1": [(0, T)], "K=70": rows}


def _spiky(T, Pn, seed):
    """randn with a few entries of 1e6 beside entries of 1e-3: another order of summation shows in the bits."""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(T, Pn, generator=g)
    u = torch.rand(T, Pn, generator=g)
    f = torch.where(u < 0.04, f.sign() * 1e6, f)
    return torch.where(u > 0.9, f * 1e-3, f).contiguous()


def _table_t(rows):
    return torch.tensor(rows, dtype=torch.int32)


@pytest.mark.parametrize("T", [1, 9, 70])
@pytest.mark.parametrize("Pn", [1, 3, 4, 5, 255, 1029, 6272])
def test_window_reduce_mean_is_the_sequential_float32_sum(dev, Pn, T):
    """op 0 against the NumPy float32 loop, bit for bit; and every element against the float64 mean under
    count * 2^-24 * mean_i |f_i|, the first-order bound of a sequential fp32 sum and one division (this one tests the
    statement, not its restatement).  P = 4 and 6272 take the 16-byte path, the others the scalar one."""
    f = _spiky(T, Pn, 100 * T + Pn)
    fd = f.to(dev)
    for name, rows in _tables(T).items():
        got = P.kernels.window_reduce(fd, _table_t(rows), "mean")
        assert got.shape == (len(rows), Pn) and got.dtype == torch.float32
        want = torch.from_numpy(R.window_mean_ref(f.numpy(), rows))
        assert torch.equal(got.cpu(), want), f"{name}: {(got.cpu() != want).sum().item()} of {want.numel()} elements differ in their bits"
        worst = 0.0
        for k, (first, count) in enumerate(rows):
            x = f[first:first + count].double()
            gate = count * 2.0 ** -24 * x.abs().mean(0)
            err = (got[k].cpu().double() - x.mean(0)).abs()
            worst = max(worst, (err / gate.clamp_min(1e-300)).max().item())
            assert bool((err <= gate).all()), f"{name} row {k} {(first, count)}: {(err / gate).max().item():.3f} of the gate"
        print(f"window_reduce mean P={Pn} T={T} {name}: worst error {worst:.3f} of the float64 gate")


def test_window_reduce_keeps_the_shape_and_takes_unaligned_rows(dev):
    """[T, Dc, h, w] in, [K, Dc, h, w] out; a tensor whose storage starts 4 bytes off a 16-byte boundary has P % 4 == 0 but
    takes the scalar path, with the same bits."""
    T, shape = 9, (32, 14, 14)
    f = _spiky(T, 32 * 14 * 14, 5).reshape(T, *shape)
    rows = _tables(T)["K=70"]
    want = torch.from_numpy(R.window_mean_ref(f.numpy(), rows))
    got = P.kernels.window_reduce(f.to(dev), _table_t(rows))
    assert got.shape == (70, *shape) and torch.equal(got.cpu(), want)
    base = torch.empty(f.numel() + 1, device=dev)
    off = base[1:].view(T, *shape)
    off.copy_(f)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    assert torch.equal(P.kernels.window_reduce(off, _table_t(rows)).cpu(), want)
    assert torch.equal(P.kernels.window_reduce(off, _table_t(rows), "max").cpu(),
                       torch.stack([f[a:a + c].amax(0) for a, c in rows]))


@pytest.mark.parametrize("T", [1, 9, 70])
@pytest.mark.parametrize("Pn", [1, 3, 4, 5, 255, 1029, 6272])
def test_window_reduce_max_equals_amax(dev, Pn, T):
    """op 1 against amax over the range, with frames that are negative throughout (a maximum started from 0 would show)."""
    f = _spiky(T, Pn, 7 * T + Pn)
    f[: (T + 1) // 2] = -f[: (T + 1) // 2].abs() - 1.0
    for name, rows in _tables(T).items():
        got = P.kernels.window_reduce(f.to(dev), _table_t(rows), "max")
        want = torch.stack([f[a:a + c].amax(0) for a, c in rows])
        assert name == "K=1" or bool((want < 0).all(1).any())                    # a row that is negative throughout
        assert torch.equal(got.cpu(), want), name


def test_window_reduce_offsets_past_two_to_the_31(dev):
    """T * P > 2^31 elements (8.9 GB): the last rows lie past what a 32-bit offset reaches.  Only the rows the table names are
    written and read."""
    T, Pn = 33, (1 << 26) + 4
    assert T * Pn > 1 << 31
    f = torch.empty(T, Pn, device=dev)
    g = torch.Generator(device=dev).manual_seed(3)
    for t in (0, T - 2, T - 1):
        f[t].normal_(generator=g)
    got = P.kernels.window_reduce(f, _table_t([(T - 2, 2), (0, 1)]), "mean")
    assert torch.equal(got[0], (f[T - 2] + f[T - 1]) / 2.0) and torch.equal(got[1], f[0])
    got = P.kernels.window_reduce(f, _table_t([(T - 2, 2)]), "max")
    assert torch.equal(got[0], torch.maximum(f[T - 2], f[T - 1]))
    del f, got
    torch.cuda.empty_cache()                                                    # the 8.9 GB go back to the card, not to the cache


# ---------------------------------------------------------------------------------------------------------------------
# whole path: one recording, one set of clips, one oracle reference per case, shared by the tests below
# ---------------------------------------------------------------------------------------------------------------------
FR, STRIDE, T_CLIP, BATCH = 700, 128, 28, 3
TOL = 3e-4          # the mask bound of test_separate_long_masks_vs_oracle_nets / test_inference_wrapper_vs_oracle


@pytest.fixture(scope="module")
def clip(dev):
    nets, onets, gen = LF._small_nets(dev, 3)
    wav = _tone_mix(HOP * (FR - 1) + 17, 6)                                  # 16 s
    with torch.no_grad():
        mag = P.kernels.Stft(dev, 1022, 256, "reflect").stft(wav.to(dev)[None])[0][0].cpu()
    assert mag.shape == (LF.FIN, FR)
    starts = S.plan_windows(FR, STRIDE)
    assert len(starts) == 5
    with torch.no_grad():
        logm = torch.log(LF.ref_resample(LF.ref_slices(mag, starts) + 1e-10, LF.FOUT, LF.W, True))
    stacks = [torch.randn(T_CLIP, 3, 64, 64, generator=gen) for _ in range(2)]
    c = types.SimpleNamespace(nets=nets, onets=onets, wav=wav, mag=mag, starts=starts, logm=logm, stacks=stacks, cache={},
                              times=torch.arange(T_CLIP, dtype=torch.float64) / 2.0,            # 2 fps: 0 ... 13.5 s
                              early=torch.arange(T_CLIP, dtype=torch.float64) / 14.0)           # all within the first 2 s
    return c


def _oracle(c, which, duet=False):
    """Per-window masks (network channel order) and attention maps of the oracle nets on the CPU: forward_multiframe over
    exactly the frames the brute-force table gives every window, relu (not for the duet), the oracle U-Net on the CPU-sliced
    windows.  Computed once per case."""
    key = (which, duet)
    if key not in c.cache:
        osnd, ofrm = c.onets
        rows = R.frames_of_windows_ref(getattr(c, which).tolist(), c.starts, RATE, HOP)
        with torch.no_grad():
            feats = []
            for st in c.stacks[:1] if duet else c.stacks:
                f = torch.cat([ofrm.forward_multiframe(st[a:a + n].permute(1, 0, 2, 3)[None], pool=False) for a, n in rows], 0)
                feats.append(f if duet else torch.relu(f))
            feat, meta = osnd(c.logm, feats * 2 if duet else feats)
            c.cache[key] = (torch.sigmoid(feat), meta[1], feats, rows)
    return c.cache[key]


def _run(c, dev, frames, times, args=None, **kw):
    with torch.no_grad():
        return S.separate_long(c.nets, c.wav.to(dev), frames, args or _args(audRate=RATE), True, STRIDE, batch=BATCH,
                               return_masks=True, frame_times=times, **kw)


def test_clip_form_masks_vs_oracle_nets(clip, dev):
    """Two stacks of 28 frames at 2 fps over 16 s (K = 5 windows): the per-window masks against the oracle within 3e-4; the
    stacks on the CPU and on the GPU give the same bits; the trunk sees every frame exactly once; the clip is not ignored."""
    c = clip
    frm = c.nets[1]
    seen, trunk = [], frm._trunk
    frm._trunk = lambda x: (seen.append(x.shape[0]), trunk(x))[1]
    try:
        on_cpu = _run(c, dev, c.stacks, c.times, return_maps=True)
        per_source = [BATCH] * (T_CLIP // BATCH) + ([T_CLIP % BATCH] if T_CLIP % BATCH else [])
        assert seen == per_source * 2 and sum(seen) == 2 * T_CLIP, seen
        on_gpu = _run(c, dev, [s.to(dev) for s in c.stacks], c.times, return_maps=True)
    finally:
        frm._trunk = trunk
    assert on_cpu["starts"] == c.starts and on_cpu["masks"].shape == (5, 2, LF.FOUT, LF.W)
    for k in ("masks", "wavs", "lin_masks", "maps"):
        assert torch.equal(on_cpu[k], on_gpu[k]), k
    assert on_cpu["perms"].tolist() == [[0, 1]] * 5 and bool(torch.isfinite(on_cpu["wavs"]).all())
    ref_masks, ref_maps, _, rows = _oracle(c, "times")
    assert [list(r) for r in rows] == S.frames_of_windows(c.times, c.starts, RATE, HOP).tolist() \
        == [[0, 12], [6, 12], [12, 12], [18, 10], [21, 7]]
    for n in range(2):
        print(f"clip form mask {n}: max|d|/max|ref| {rel_err(on_cpu['masks'][:, n], ref_masks[:, n]):.3e}")
        assert_close(on_cpu["masks"][:, n], ref_masks[:, n], TOL, f"clip form mask {n}")
    print(f"clip form maps: max|d|/max|ref| {rel_err(on_cpu['maps'], ref_maps):.3e}")
    assert on_cpu["maps"].shape == ref_maps.shape
    assert_close(on_cpu["maps"], ref_maps, TOL, "attention maps")                # the bound test_inference_wrapper_vs_oracle holds maps to
    # one shared frame per source is another separation
    with torch.no_grad():
        first = S.separate_long(c.nets, c.wav.to(dev), [s[:1].to(dev) for s in c.stacks], _args(audRate=RATE), True, STRIDE,
                                batch=BATCH, return_masks=True)
    moved = rel_err(first["masks"], on_cpu["masks"])
    print(f"clip form vs the first frame alone: max|d|/max {moved:.3e}")
    assert moved > TOL


def test_clip_form_empty_windows_take_the_nearest_frame(clip, dev):
    """All 28 frames within the first two seconds: windows 1 ... 4 hold none and are separated with the frame nearest to
    them, the last one."""
    c = clip
    out = _run(c, dev, c.stacks, c.early)
    ref_masks, _, _, rows = _oracle(c, "early")
    assert rows == [(0, 28)] + [(27, 1)] * 4
    for n in range(2):
        print(f"empty windows mask {n}: max|d|/max|ref| {rel_err(out['masks'][:, n], ref_masks[:, n]):.3e}")
        assert_close(out["masks"][:, n], ref_masks[:, n], TOL, f"empty-window mask {n}")


def test_clip_form_refusals(clip, dev):
    c = clip
    E = P.lib.AvsepError
    with pytest.raises(E):
        _run(c, dev, c.stacks, c.times[:-1])                                    # one time per frame
    with pytest.raises(E):
        _run(c, dev, c.stacks, c.times.flip(0))                                 # decreasing times
    with pytest.raises(E):
        _run(c, dev, [c.stacks[0], c.stacks[1][:5]], c.times)                   # stacks of equal shape
    with pytest.raises(E):
        _run(c, dev, c.stacks[:1], c.times, args=_args(audRate=RATE, num_mix=3))      # a duet has two sources
    with pytest.raises(E):
        _run(c, dev, c.stacks, c.times, args=_args(audRate=RATE, not_pool_vis=True), return_maps=True)
    with pytest.raises(E, match="pooled"):
        _run(c, dev, c.stacks, c.times, args=_args(audRate=RATE, not_pool_vis=True))      # the fusion takes maps only
    with pytest.raises(E):
        with torch.no_grad():
            S.separate_long(c.nets, c.wav.to(dev), None, _args(audRate=RATE), False, STRIDE, return_maps=True)
    with pytest.raises(NotImplementedError):
        _run(c, dev, c.stacks, c.times, args=_args(audRate=RATE, fusion_type="MixVis"))


@pytest.mark.parametrize("pool_type,op", [("maxpool", "max"), ("avgpool", "mean")])
def test_pooled_features_per_window_vs_oracle_multiframe(clip, dev, pool_type, op):
    """The fusion of these nets (as the reference's) takes spatial maps only, so separate_long refuses pooled features in the
    clip form (test_clip_form_refusals) and window_reduce is tested on [T, Dc] alone: the per-frame pooled vectors of the HIP
    trunk through window_reduce (max for maxpool, mean for avgpool) against the oracle's forward_multiframe(pool=True) over
    each window's frames (3e-4, the bound test_visual_eval holds the pooled trunk output to)."""
    c = clip
    frm, ofrm = c.nets[1], c.onets[1]
    rows = R.frames_of_windows_ref(c.times.tolist(), c.starts, RATE, HOP)
    keep = frm.pool_type, ofrm.pool_type
    frm.pool_type = ofrm.pool_type = pool_type
    try:
        with torch.no_grad():
            st = c.stacks[0]
            per_frame = frm.forward(st.to(dev), pool=True).float().contiguous()
            assert per_frame.shape == (T_CLIP, 32)
            got = P.kernels.window_reduce(per_frame, _table_t(rows), op)
            want = torch.cat([ofrm.forward_multiframe(st[a:a + n].permute(1, 0, 2, 3)[None], pool=True) for a, n in rows], 0)
    finally:
        frm.pool_type, ofrm.pool_type = keep
    print(f"pooled {pool_type}: max|d|/max|ref| {rel_err(got, want):.3e}")
    assert got.shape == want.shape == (5, 32)
    assert_close(got, want, TOL, f"pooled {pool_type} window features")


def test_duet_clip_masks_alignment_and_maps(clip, dev):
    """One stack for both sources.  Masks in network channel order against oracle.inference.forward's duet form fed the
    window-mean features (3e-4); perms equal align_permutations of a float64 agreement computed from the GPU's own masks;
    lin_masks are the float64 blend under those perms (1e-5); maps[k, n] is the oracle's att_maps[k, perms[k][n]] (1e-5)."""
    c = clip
    out = _run(c, dev, c.stacks[:1], c.times, return_maps=True)
    _, _, feats, _ = _oracle(c, "times", duet=True)
    fed = types.SimpleNamespace(forward=lambda x, pool: x)                      # the window-mean features go in as they are
    with torch.no_grad():
        ref = OI.forward((c.onets[0], fed), (LF.ref_slices(c.mag, c.starts), None), [feats[0]], _args(audRate=RATE), True)
    masks = out["masks"].cpu()
    for n in range(2):
        print(f"duet mask {n}: max|d|/max|ref| {rel_err(masks[:, n:n + 1], ref['pred_masks'][n]):.3e}")
        assert_close(masks[:, n:n + 1], ref["pred_masks"][n], TOL, f"duet mask {n}")
    D = LF.ref_agreement(masks, c.starts)
    perms = S.align_permutations(D)
    margins = []
    for k in range(D.shape[0]):
        cur = perms[k].tolist()
        costs = sorted(sum(D[k, cur[n], p[n]].item() for n in range(2)) for p in ((0, 1), (1, 0)))
        margins.append((costs[1] - costs[0]) / costs[1])
    print(f"duet alignment: perms {perms.tolist()}, least margin between the candidates {min(margins):.3e} of the cost")
    assert min(margins) >= 1e-3, "a near tie between the candidates: pick another seed"
    assert out["perms"].tolist() == perms.tolist()
    assert_close(out["lin_masks"], LF.ref_stitch(masks, c.starts, perms.tolist(), FR), 1e-5, "duet blended masks")
    want = torch.stack([ref["maps"][k, perms[k].long()] for k in range(5)])
    print(f"duet maps: max|d|/max|ref| {rel_err(out['maps'], want):.3e}")
    assert out["maps"].shape == want.shape == (5, 2, 4, 4)
    assert_close(out["maps"], want, 1e-5, "duet maps")


def test_duet_in_the_old_frame_forms_runs(clip, dev):
    c = clip
    args = _args()
    with torch.no_grad():
        one = S.separate_long(c.nets, c.wav.to(dev), [c.stacks[0][:1].to(dev)], args, True, STRIDE, return_masks=True, return_maps=True)
        per = S.separate_long(c.nets, c.wav.to(dev), [c.stacks[0][:5].to(dev)], args, True, STRIDE, return_masks=True)
    for out in (one, per):
        assert out["masks"].shape == (5, 2, LF.FOUT, LF.W) and out["perms"].shape == (5, 2) and out["perms"][0].tolist() == [0, 1]
        assert bool(torch.isfinite(out["wavs"]).all()) and out["wavs"].abs().max().item() > 1e-3
    assert one["maps"].shape == (5, 2, 4, 4)
    # maps follow the sources: under another alignment, maps[k, n] is the map of channel perms[k][n]
    table = torch.tensor([[0, 1], [1, 0], [1, 0], [0, 1], [1, 0]], dtype=torch.int32)
    keep = S.align_permutations
    S.align_permutations = lambda D: table
    try:
        with torch.no_grad():
            swapped = S.separate_long(c.nets, c.wav.to(dev), [c.stacks[0][:1].to(dev)], args, True, STRIDE, return_maps=True)
    finally:
        S.align_permutations = keep
    assert swapped["perms"].tolist() == table.tolist()
    for k in range(5):
        network_order = one["maps"][k][one["perms"][k].long()]                  # a permutation of two is its own inverse
        assert torch.equal(swapped["maps"][k], network_order[table[k].long()])
    assert not torch.equal(one["maps"][:, 0], one["maps"][:, 1])
    # img_activation is not applied to a duet's map: the same frame as two sources' frames is another separation
    with torch.no_grad():
        two = S.separate_long(c.nets, c.wav.to(dev), [c.stacks[0][:1].to(dev)] * 2, args, True, STRIDE, return_masks=True)
    assert rel_err(one["masks"], two["masks"]) > TOL
    with pytest.raises(P.lib.AvsepError):
        S.separate_long(c.nets, c.wav.to(dev), [c.stacks[0][:1].to(dev)], _args(num_mix=3), True, STRIDE)


def test_frame_times_none_is_the_earlier_path(clip, dev):
    c = clip
    args = _args()
    wav = c.wav.to(dev)
    for frames in ([s[:1].to(dev) for s in c.stacks], [s[:5].to(dev) for s in c.stacks]):
        with torch.no_grad():
            a = S.separate_long(c.nets, wav, frames, args, True, STRIDE, batch=2, return_masks=True)
            b = S.separate_long(c.nets, wav, frames, args, True, STRIDE, batch=2, return_masks=True, frame_times=None, return_maps=False)
        assert sorted(a) == sorted(b) and "maps" not in b
        for k in ("wavs", "masks", "perms", "lin_masks"):
            assert torch.equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_separates_with_clips_and_writes_maps(dev, tmp_path):
    """python -m avsep_amd.separate in process: a short WAV and two stacks with --fps 2 --maps, then one stack, the duet."""
    mb = P.ModelBuilder()
    torch.manual_seed(11)
    snd = mb.build_sound(arch="unet5", fc_dim=2, fusion_type="hidsep", att_type="sig")
    frm = mb.build_frame(arch="resnet18dilated", fc_dim=256, pool_type="maxpool")
    torch.save(snd.state_dict(), str(tmp_path / "sound.pth"))
    torch.save(frm.state_dict(), str(tmp_path / "frame.pth"))
    L = 30000
    S.write_wav(str(tmp_path / "mix.wav"), _tone_mix(L, 8).numpy(), RATE)
    g = torch.Generator().manual_seed(3)
    paths = []
    for n in range(2):
        np.save(str(tmp_path / f"f{n}.npy"), torch.randn(5, 3, 64, 64, generator=g).numpy())
        paths.append(str(tmp_path / f"f{n}.npy"))
    common = ["--wav", str(tmp_path / "mix.wav"), "--fps", "2", "--maps", "--arch_sound", "unet5", "--num_channels", "2",
              "--vis_channels", "256", "--img_pool", "maxpool", "--not_pool_vis", "--fusion_type", "hidsep", "--att_type", "sig",
              "--binary_mask", "0", "--weights_sound", str(tmp_path / "sound.pth"), "--weights_frame", str(tmp_path / "frame.pth")]
    for files, name in ((paths, "two"), (paths[:1], "duet")):
        outdir = tmp_path / name
        out = S.cli(common + ["--frames", *files, "--out", str(outdir)])
        maps = np.load(str(outdir / "maps.npy"))
        assert maps.shape == (1, 2, 4, 4) and maps.dtype == np.float32 and np.isfinite(maps).all()
        assert np.array_equal(maps, out["maps"].cpu().numpy())
        for n in range(2):
            x, rate = S.read_wav(str(outdir / f"source{n}.wav"))
            assert rate == RATE and x.shape == (HOP * (L // HOP),) and np.isfinite(x).all() and np.abs(x).max() > 1e-3
        assert sorted(p.name for p in outdir.iterdir()) == ["maps.npy", "source0.wav", "source1.wav"]
