"""Evaluation visuals: what a run has learnt, as a page one can look at and listen to (the reference's main.py:290-418
``output_visuals``, utils.py:81-98 and the page of viz.py, which go through NumPy, OpenCV, imageio and ffmpeg item by item).

Every image of a batch is rendered by ONE kernel body, ``avsep_spec_image`` (include/avsep.h; ``kernels.spec_image``): mask
product, log scale, 8-bit level, JET colours and the row flip on the way from one read of the magnitudes to the bytes a file
takes.  A batch of B items and N sources is a handful of launches, not 2 + 4N images times B round trips:

    mix            log10(outputs["mag_mix"] + 1) * 200, JET           (the warped mixture the network saw)
    weight         outputs["weight"] * 100, JET
    predamp{n}     log10(batch["mag_mix"] * predicted linear mask + 1) * 200, JET; the threshold is taken inside the kernel
    gtamp{n}       the same with the true mask
    predmask{n}    clip(predicted mask, 0, 1) * 255, grey (warped, thresholded first under --binary_mask)
    gtmask{n}      the same with the true mask

``output_visuals`` lays the files of the first ``num_vis`` validation items out as the reference does (one folder per item
id under <vis>/av or <vis>/ao: .jpg images through Pillow, 24-bit .wav files through wavio), with one ``frames{n}.png``
strip of the item's frames in place of the reference's ffmpeg videos; ``write_page`` writes the table that shows them.
With ``args.gpu_encode`` (``train.py --gpu_encode``) the .jpg images stay on the device and ``jpeg.encode`` writes them in one
call: the same bytes as Pillow's, and only those bytes cross to the host; the PNG strips stay with Pillow.

``report`` is the same picture for a recording of any length (``separate --report``): the mixture, every stem's share of it
and every stitched mask at ``cell = ceil(frames / width)`` STFT frames per image column.
"""
import html
import os

import torch

from . import kernels as K
from . import lib
from .lib import AvsepError

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
IMG_STYLE = "max-height:256px;max-width:256px;"
PNG = {"compress_level": 1}     # zlib's fastest: the encode, not the rendering, is what a picture costs


def _pillow(what):
    try:
        from PIL import Image
    except ImportError as e:
        raise AvsepError(f"{what} writes its images through Pillow, which is not installed") from e
    return Image


_TABLES = {}


def jet(device):
    """localise.jet_table() on ``device``, uploaded once per device."""
    device = torch.device(device)
    if device not in _TABLES:
        from .localise import jet_table
        _TABLES[device] = torch.from_numpy(jet_table()).to(device)
    return _TABLES[device]


# ---------------------------------------------------------------------------------------------------------------------
# the images of a batch
# ---------------------------------------------------------------------------------------------------------------------
def _planes(masks, items=None):
    """A list of N masks [B,1,F,T] (views or not) -> one dense f32 [N*B,F,T]; items: only the first ``items`` of the B."""
    return torch.stack([m.detach().float()[:items, 0] for m in masks], 0).flatten(0, 1).contiguous()


def linear_masks(outputs, args, Fin, items=None):
    """-> (pred, gt): f32 [N*B,Fin,T] each, the masks on the STFT's own rows: un-warped when args.log_freq
    (``kernels.warp(..., 0)``, main.py:313-321), one launch for the predicted and the true masks of every source.
    items: only the first ``items`` of the batch (B is then ``items``)."""
    N = args.num_mix
    both = torch.cat([_planes(outputs["pred_masks"][:N], items), _planes(outputs["gt_masks"][:N], items)], 0)     # [2*N*B, Fw, T]
    if args.log_freq:
        both = K.warp(both[:, None].contiguous(), Fin, both.shape[2], 0)[:, 0]
    pred, gt = both[:both.shape[0] // 2], both[both.shape[0] // 2:]
    return pred.contiguous(), gt.contiguous()


def _weight_plane(outputs, items=None):
    """outputs["weight"]: [B,1,F,T] like "mag_mix" from the audio-visual pass, [B,F,T,S] (S copies of it) from the audio-only
    one -> [B,F,T]."""
    w = outputs["weight"].detach().float()
    return (w[:items, 0] if w.shape == outputs["mag_mix"].shape else w[:items, ..., 0]).contiguous()


def item_images(batch, outputs, args, items=None, linear=None):
    """Every image main.py:352-386 saves for the B items of a batch -> {name: uint8 tensor on the device}, row 0 on top:
    "mix", "weight" [B,Fw,T,3]; "predamp{n}", "gtamp{n}" [B,Fin,T,3]; "predmask{n}", "gtmask{n}" [B,Fw,T] (grey), n from 1.
    batch: "mag_mix" [B,1,Fin,T]; outputs: NetWrapper.forward's.  Nothing in either is changed.
    items: only the first ``items`` of the batch are rendered (B is then ``items``); linear: ``linear_masks`` of the same
    outputs, args and items where the caller has them already."""
    mag = batch["mag_mix"]
    lib.require_gpu(mag)
    N, Fin = args.num_mix, mag.shape[2]
    mag = mag.detach().float()[:items, 0].contiguous()                          # [B,Fin,T]
    B = mag.shape[0]
    table = jet(mag.device)
    thres = float(args.mask_thres) if args.binary_mask else None
    out = {"mix": K.spec_image(outputs["mag_mix"].detach().float()[:items, 0].contiguous(), table=table),
           "weight": K.spec_image(_weight_plane(outputs, items), log=False, scale=100.0, table=table)}
    pred_lin, gt_lin = linear if linear is not None else linear_masks(outputs, args, Fin, items)
    mags = mag[None].expand(N, -1, -1, -1).reshape(N * B, Fin, -1).contiguous()
    amp = {"predamp": K.spec_image(mags, pred_lin, thres, table=table), "gtamp": K.spec_image(mags, gt_lin, table=table)}
    pred_w, gt_w = _planes(outputs["pred_masks"][:N], items), _planes(outputs["gt_masks"][:N], items)
    if args.binary_mask:                                                        # on the warped mask, as main.py:336 does
        pred_w = (pred_w > args.mask_thres).float()
    grey = K.spec_image(torch.cat([pred_w, gt_w], 0), log=False, scale=255.0)[..., 0]
    for n in range(N):
        out[f"predamp{n + 1}"] = amp["predamp"][n * B:(n + 1) * B]
        out[f"gtamp{n + 1}"] = amp["gtamp"][n * B:(n + 1) * B]
        out[f"predmask{n + 1}"] = grey[n * B:(n + 1) * B]
        out[f"gtmask{n + 1}"] = grey[(N + n) * B:(N + n + 1) * B]
    return out


def frame_strips(frames):
    """One source's normalised frames [B,3,T,H,W] -> uint8 [B,H,T*W,3]: the T frames side by side, back on 0..255 rounded and
    clamped (utils.py:81-87 truncates and wraps)."""
    f = frames.detach().float()
    mean, std = (torch.tensor(v, dtype=torch.float32, device=f.device).view(1, 3, 1, 1, 1) for v in (MEAN, STD))
    u8 = ((f * std + mean) * 255.0).round_().clamp_(0.0, 255.0).to(torch.uint8)
    B, _, T, H, W = u8.shape
    return u8.permute(0, 3, 2, 4, 1).reshape(B, H, T * W, 3).contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# the page
# ---------------------------------------------------------------------------------------------------------------------
def write_page(path, header, rows, note=None):
    """``index.html``: a table with one header row (``header``: the column titles) and one row per entry of ``rows``.  A row is
    a list of cells; a cell is a dict with any of "text" (a string, or a list of lines), "image" and "audio" (paths relative
    to the page).  Everything is escaped."""
    esc = lambda s: html.escape(str(s), quote=True)   # noqa: E731
    out = ["<!DOCTYPE html>", "<html><head><meta charset=\"utf-8\">",
           "<style>table, th, td {border: 1px solid #444; border-collapse: collapse; padding: 4px; font-family: sans-serif;}"
           "</style></head><body>"]
    if note:
        out.append(f"<p>{esc(note)}</p>")
    out.append("<table>")
    out.append("<tr>" + "".join(f"<th>{esc(h)}</th>" for h in header) + "</tr>")
    for row in rows:
        cells = []
        for cell in row:
            parts = []
            if "text" in cell:
                lines = cell["text"] if isinstance(cell["text"], (list, tuple)) else [cell["text"]]
                parts.append("<br>".join(esc(line) for line in lines))
            if "image" in cell:
                parts.append(f"<img src=\"{esc(cell['image'])}\" style=\"{IMG_STYLE}\">")
            if "audio" in cell:
                parts.append(f"<audio controls preload=\"none\"><source src=\"{esc(cell['audio'])}\"></audio>")
            cells.append("<td>" + "<br>".join(parts) + "</td>")
        out.append("<tr>" + "".join(cells) + "</tr>")
    out.append("</table></body></html>")
    with open(path, "w", encoding="utf-8") as f:
        f.write("\n".join(out) + "\n")


def page_header(N):
    head = ["item", "mixture"]
    for n in range(1, N + 1):
        head += [f"frames {n}", f"predicted {n}", f"true {n}", f"predicted mask {n}", f"true mask {n}"]
    return head + ["loss weight"]


def write_index(vis_rows, args, use_vis):
    """The page of the rows ``output_visuals`` collected: <vis>/av/index.html or <vis>/ao/index.html."""
    root = os.path.join(args.vis, "av" if use_vis else "ao")
    os.makedirs(root, exist_ok=True)
    write_page(os.path.join(root, "index.html"), page_header(args.num_mix), vis_rows)
    return os.path.join(root, "index.html")


# ---------------------------------------------------------------------------------------------------------------------
# the files of a batch
# ---------------------------------------------------------------------------------------------------------------------
def _write_wav(path, wav, rate):
    """f32 [L] on the GPU -> mono 24-bit PCM (the reference's subtype='PCM_24'); the kernel rounds and packs the bytes."""
    from . import resample as R
    from . import wavio
    raw = R.join_frames(wav.detach().float()[None].contiguous(), rate, rate, "s24")
    wavio.write_frames(path, raw.cpu().numpy(), rate, 1, "s24")


def _folder(item_id):
    """An item's id as one path component."""
    name = str(item_id).replace(os.sep, "-").replace("/", "-").strip() or "item"
    return "item" if name in (".", "..") else name


def output_visuals(vis_rows, batch, outputs, args, metrics, use_vis, stft_plan=None):
    """main.py:290-418 for the items of one batch that still fit under ``args.num_vis``: their folders under
    <args.vis>/av (use_vis) or <args.vis>/ao, and one row per item appended to ``vis_rows`` for ``write_index``.
    metrics: evaluate.calc_metrics' result for the same batch ("pred_wavs" [N,B,L]; "sdr" / "sir" [B,N] where it has them).
    args.gpu_encode (optional): the .jpg files are encoded on the GPU, byte for byte the files Pillow writes.
    Returns the number of items written."""
    Image = _pillow("output_visuals")
    mag_mix, phase = batch["mag_mix"], batch["phase_mix"]
    lib.require_gpu(mag_mix)
    N, B = args.num_mix, mag_mix.shape[0]
    todo = min(B, max(0, int(args.num_vis) - len(vis_rows)))
    if todo == 0:
        return 0
    root = os.path.join(args.vis, "av" if use_vis else "ao")
    os.makedirs(root, exist_ok=True)
    with torch.no_grad():                                                       # only the ``todo`` items that are written
        mag = mag_mix.detach().float()[:todo, 0].contiguous()
        ph = phase.detach().float()[:todo, 0].contiguous()
        linear = linear_masks(outputs, args, mag.shape[1], todo)                # one un-warp for the pictures and the sounds
        images = item_images(batch, outputs, args, todo, linear)
        if getattr(args, "gpu_encode", False):                                  # the .jpg files of all items in one encode
            from . import jpeg
            names = ["mix", "weight"] + [f"{kind}{n}" for n in range(1, N + 1) for kind in ("predamp", "gtamp", "predmask", "gtmask")]
            files = jpeg.encode([images[k][j] for j in range(todo) for k in names])
            jpgs = [dict(zip(names, files[j * len(names):(j + 1) * len(names)])) for j in range(todo)]
        else:
            images = {k: v.cpu().numpy() for k, v in images.items()}
            jpgs = None
        plan = stft_plan or K.Stft(mag_mix.device, args.stft_frame, args.stft_hop, getattr(args, "stft_pad_mode", "reflect"))
        gt_mag = (mag[None] * linear[1].view(N, todo, *mag.shape[1:])).reshape(N * todo, *mag.shape[1:]).contiguous()
        waves = plan.istft(torch.cat([mag, gt_mag], 0), ph.repeat(N + 1, 1, 1)).clamp_(-1.0, 1.0)      # mix, then gt [N,todo]
        strips = [frame_strips(f[:todo]).cpu().numpy() for f in batch["frames"][:N]] if "frames" in batch else None
    pred_wavs = metrics["pred_wavs"]
    for j in range(todo):
        name = _folder(batch["id"][j])
        os.makedirs(os.path.join(root, name), exist_ok=True)
        rel = lambda fn: name + "/" + fn                                        # noqa: E731
        full = lambda fn: os.path.join(root, name, fn)                          # noqa: E731

        def save_jpg(key):
            if jpgs is None:
                Image.fromarray(images[key][j]).save(full(key + ".jpg"))
            else:
                with open(full(key + ".jpg"), "wb") as f:
                    f.write(jpgs[j][key])
        save_jpg("mix")
        save_jpg("weight")
        _write_wav(full("mix.wav"), waves[j], args.audRate)
        text = [name]
        for key in ("sdr", "sir"):
            if key in metrics:
                text.append(key.upper() + ": " + ", ".join(f"{float(v):.2f}" for v in metrics[key][j]))
        row = [{"text": text}, {"image": rel("mix.jpg"), "audio": rel("mix.wav")}]
        for n in range(1, N + 1):
            for kind in ("predamp", "gtamp", "predmask", "gtmask"):
                save_jpg(f"{kind}{n}")
            _write_wav(full(f"pred{n}.wav"), pred_wavs[n - 1, j], args.audRate)
            _write_wav(full(f"gt{n}.wav"), waves[n * todo + j], args.audRate)
            cell = {"text": "audio only"}
            if strips is not None:
                Image.fromarray(strips[n - 1][j]).save(full(f"frames{n}.png"), **PNG)
                cell = {"image": rel(f"frames{n}.png")}
            row += [cell, {"image": rel(f"predamp{n}.jpg"), "audio": rel(f"pred{n}.wav")},
                    {"image": rel(f"gtamp{n}.jpg"), "audio": rel(f"gt{n}.wav")},
                    {"image": rel(f"predmask{n}.jpg")}, {"image": rel(f"gtmask{n}.jpg")}]
        row.append({"image": rel("weight.jpg")})
        vis_rows.append(row)
    return todo


# ---------------------------------------------------------------------------------------------------------------------
# a recording of any length
# ---------------------------------------------------------------------------------------------------------------------
REPORT_NOTE = ("Stem pictures are the stitched mask times the mixture's STFT magnitude, before any Wiener filter or phase "
               "iteration; with --channels keep they show the down-mix the model heard.  Low frequencies are at the bottom.")
BINARY_NOTE = ("  The stems were made with a binary mask: their pictures use the stitched mask thresholded at {thres:g}, as "
               "the stems do; the mask pictures show it before the threshold.")


def report_cell(frames, width):
    """STFT frames per image column so that ``frames`` of them fit into ``width`` pixels."""
    if int(width) < 1:
        raise AvsepError(f"the report's width is a positive number of pixels, got {width!r}")
    return max(1, -(-int(frames) // int(width)))


def report_images(mag, lin_masks, width, thres=None):
    """mag f32 [Fin,F], the mixture's STFT magnitude; lin_masks f32 [N,Fin,F] (separate_long(return_masks=True)) ->
    (mix uint8 [Fin,W,3], sources uint8 [N,Fin,W,3], masks uint8 [N,Fin,W], cell), W = ceil(F / cell): the maximum over a
    cell for the spectrograms, the mean for the masks.  thres: the threshold the stems' binary mask took (None: the soft
    mask), so that a source's picture is mag * (M > thres) as its stem is (mask_stitch); the mask pictures stay M.
    Three launches."""
    lib.require_gpu(mag)
    N = lin_masks.shape[0]
    cell = report_cell(mag.shape[1], width)
    table = jet(mag.device)
    mag = mag.detach().float().contiguous()
    lin = lin_masks.detach().float().contiguous()
    mix = K.spec_image(mag[None], cell=cell, table=table)[0]
    src = K.spec_image(mag[None].expand(N, -1, -1).contiguous(), lin, thres, cell=cell, table=table)
    msk = K.spec_image(lin, cell=cell, reduce="mean", log=False, scale=255.0)[..., 0]
    return mix, src, msk, cell


def report(out_dir, wav, lin_masks, args, width=2048, title=None):
    """<out_dir>/report.html with mix.png, source{n}.png and mask{n}.png for one separated recording.  wav f32 [L] on the
    GPU: what the model heard.  Returns the cell."""
    Image = _pillow("--report")
    with torch.no_grad():
        plan = K.Stft(wav.device, args.stft_frame, args.stft_hop, getattr(args, "stft_pad_mode", "reflect"))
        mag = plan.stft(wav.float().contiguous()[None], want_phase=False)[0][0].contiguous()
        thres = float(getattr(args, "mask_thres", 0.5)) if args.binary_mask else None      # separate_long's own reading
        mix, src, msk, cell = report_images(mag, lin_masks, width, thres)
    os.makedirs(out_dir, exist_ok=True)
    Image.fromarray(mix.cpu().numpy()).save(os.path.join(out_dir, "mix.png"), **PNG)
    row = [{"text": title or "recording"}, {"image": "mix.png"}]
    head = ["recording", "mixture"]
    src, msk = src.cpu().numpy(), msk.cpu().numpy()
    for n in range(src.shape[0]):
        Image.fromarray(src[n]).save(os.path.join(out_dir, f"source{n}.png"), **PNG)
        Image.fromarray(msk[n]).save(os.path.join(out_dir, f"mask{n}.png"), **PNG)
        stem = os.path.join(out_dir, f"source{n}.wav")
        cellm = {"image": f"source{n}.png"}
        if os.path.exists(stem):
            cellm["audio"] = f"source{n}.wav"
        row += [cellm, {"image": f"mask{n}.png"}]
        head += [f"source {n}", f"mask {n}"]
    seconds = args.stft_hop * cell / float(args.audRate)
    write_page(os.path.join(out_dir, "report.html"), head, [row],
               note=REPORT_NOTE + (BINARY_NOTE.format(thres=thres) if thres is not None else "")
               + f"  One image column is {cell} STFT frame{'s' if cell != 1 else ''} ({seconds:.3f} s): "
                                  f"the maximum over them in the spectrograms, the mean in the masks.")
    return cell
