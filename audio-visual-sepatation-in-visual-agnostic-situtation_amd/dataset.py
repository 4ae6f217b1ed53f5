"""Input-pipeline contract (reference: dataset/base.py:17-215, dataset/music.py:52-331,
dataset/video_transforms.py).

``MUSICMixDataset(csv_path, params, split=..., seed=..., random_sample=..., vis_data=...)`` reads the reference's
6-column lists (``audio.wav, frame_dir, num_frames, fps, audio_seconds, class``; rows with < 2 fields skipped),
repeats / shuffles them like the reference and draws a mixture per index with the SAME sequence of ``random``
calls (``random.seed(index)`` first), so the chosen clips, centre times, per-source gains and frame file names are
those the reference would draw:

* partner selection ``dc`` / ``sc`` / ``sv`` / ``random`` / ``vis1`` (music.py:56-92) and the chained
  ``random.random()`` strategy draw (music.py:283-289);
* centre time ~ U(start, end) with the margin rule, up to 10 tries against silence (music.py:96-130);
* window cut, U(0.5,1.5) gain in train, clip to +-1, divide by N, mixture = sum (base.py:156-172, music.py:120,127);
* frame indices ``round(t*fps) + (i - T//2)*stride`` or the ``one_frame`` random shift (music.py:132-156);
* frames: bicubic resize (shorter side to 1.1*imgSize in train, imgSize in val; long side capped at 448),
  random/centre crop, random flip (train), /255, ImageNet mean/std, stacked to [3,T,H,W] (base.py:96-110).

What is different, on purpose: the loader does NOT run the STFT (base.py:142-147 does it with librosa on the CPU
workers) — batches carry waveforms and ``NetWrapper.attach_stft`` computes mag/phase on the GPU; ``collate``
stacks into pinned host memory for asynchronous H2D copies.  Decoding uses ``scipy.io.wavfile`` (+ polyphase
resampling when the file's rate differs from audRate; librosa's resampler is not in this image) and PIL.
"""
import csv
import os
import random

import numpy as np
import torch

MUSIC11_CLASSES = ["accordion", "acoustic_guitar", "cello", "clarinet", "erhu", "flute", "saxophone", "trumpet",
                   "tuba", "violin", "xylophone"]
_MEAN, _STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def read_list(csv_path):
    with open(csv_path, "r") as f:
        return [row for row in csv.reader(f, delimiter=",") if len(row) >= 2]


# ------------------------------------------------------------------------------------------ decoding
def read_wav_segment(path, rate, offset, duration):
    """Mono float32 samples of [offset, offset+duration) seconds at `rate` (librosa.load(sr, mono, offset, duration))."""
    from scipy.io import wavfile
    sr, data = wavfile.read(path, mmap=True)
    a, b = int(round(max(offset, 0.0) * sr)), int(round((max(offset, 0.0) + duration) * sr))
    seg = np.asarray(data[a:b])
    if seg.dtype.kind == "i":
        seg = seg.astype(np.float32) / float(np.iinfo(seg.dtype).max + 1)
    elif seg.dtype.kind == "u":
        seg = (seg.astype(np.float32) - 128.0) / 128.0
    else:
        seg = seg.astype(np.float32)
    if seg.ndim == 2:
        seg = seg.mean(axis=1)
    if sr != rate and len(seg):
        from math import gcd
        from scipy.signal import resample_poly
        g = gcd(int(sr), int(rate))
        seg = resample_poly(seg, rate // g, sr // g).astype(np.float32)
    return seg, rate


def _resize_size(w, h, size, max_size):
    # torchvision.transforms.functional.resize with an int size: shorter side -> size, long side capped at max_size
    short, long_ = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long_ / short)
    if max_size is not None and new_long > max_size:
        new_short, new_long = int(max_size * new_short / new_long), max_size
    return (new_short, new_long) if w <= h else (new_long, new_short)


def draw_crop_flip(w, h, img_size, train):
    """The one statement of a clip's crop and flip draws, for a first frame resized to w x h -> ((i, j) | None, flip).
    Training form: randint(0, h - S), randint(0, w - S) (neither when the frame is S x S already), then random() for the flip,
    in this order; a frame smaller than the crop raises randint's ValueError.  Validation form: no draw, (None, False): every
    frame takes its own centre."""
    if not train:
        return None, False
    if w == img_size and h == img_size:
        i = j = 0
    else:
        i = random.randint(0, h - img_size)
        j = random.randint(0, w - img_size)
    return (i, j), random.random() < 0.5


class VideoTransform:
    """The reference's Compose of video_transforms (one crop / flip decision per clip, shared by its frames)."""

    def __init__(self, img_size, train, max_size=448):
        self.img_size, self.train, self.max_size = img_size, train, max_size

    def resized_size(self, w, h):
        """The size a w x h frame is resized to, (w', h')."""
        return _resize_size(w, h, int(self.img_size * 1.1) if self.train else self.img_size, self.max_size)

    def __call__(self, frames):
        from PIL import Image
        frames = [f.resize(self.resized_size(f.size[0], f.size[1]), Image.BICUBIC) for f in frames]
        th = tw = self.img_size
        w, h = frames[0].size
        crop, flip = draw_crop_flip(w, h, self.img_size, self.train)
        if self.train:
            i, j = crop
            frames = [f.crop((j, i, j + tw, i + th)) for f in frames]
            if flip:
                frames = [f.transpose(Image.FLIP_LEFT_RIGHT) for f in frames]
        else:
            out = []
            for f in frames:
                w, h = f.size
                i, j = int(round((h - th) / 2.0)), int(round((w - tw) / 2.0))
                out.append(f.crop((j, i, j + tw, i + th)))
            frames = out
        mean = torch.tensor(_MEAN).view(3, 1, 1)
        std = torch.tensor(_STD).view(3, 1, 1)
        ts = [(torch.from_numpy(np.asarray(f, dtype=np.uint8).copy()).permute(2, 0, 1).float().div_(255.0) - mean) / std
              for f in frames]
        return torch.stack(ts, dim=1)                                   # [3,T,H,W]


# ------------------------------------------------------------------------------------------ dataset
class MUSICMixDataset(torch.utils.data.Dataset):
    def __init__(self, csv_path, params, split="val", debug=False, seed=None, random_sample=False, vis_data=False,
                 raw_frames=False, jpeg_bytes=False):
        p = params
        self.debug = debug
        self.raw_frames = bool(raw_frames)     # items carry the decoded uint8 frames and the draws: to_device prepares them on the GPU
        self.jpeg_bytes = bool(jpeg_bytes)     # ... the files' bytes instead of the decoded frames: to_device decodes them too (jpeg.decode)
        if self.jpeg_bytes and not self.raw_frames:
            raise ValueError("MUSICMixDataset(jpeg_bytes=True) is a form of raw_frames=True: pass both")
        self.num_frames, self.imgSize, self.stride_frames = p["num_frames"], p["imgSize"], p["stride_frames"]
        self.one_frame = p["one_frame"]
        if p.get("load_clips"):
            raise NotImplementedError("load_clips (mmaction clip pipeline for net_motion) is out of scope")
        self.audRate, self.audLen = p["audRate"], p["audLen"]
        self.audSec = 1.0 * self.audLen / self.audRate
        self.num_mix = p["num_mix"]
        self.classes = MUSIC11_CLASSES
        self.rate_dc, self.rate_sc, self.rate_sv = p["rate_dc"], p["rate_sc"], p["rate_sv"]
        self.margin, self.max_silent = p["margin"], p["max_silent"]
        self.class_int_map = {k: v for v, k in enumerate(self.classes)}
        self.split = split
        self.seed = seed if seed is not None else p["seed"]
        self.random_sample, self.vis_data = random_sample, vis_data
        random.seed(self.seed)
        self.vid_transform = VideoTransform(self.imgSize, split == "train")
        if isinstance(csv_path, str):
            self.list_samples = read_list(csv_path)
        elif isinstance(csv_path, list):
            self.list_samples = csv_path
        else:
            raise TypeError("Error list_samples!")
        print(f"Length of dataset: {len(self.list_samples)}")
        self.dict_samples = {}
        for s in self.list_samples:
            self.dict_samples.setdefault(s[-1], []).append(s)
        if split == "train":
            self.list_samples = self.list_samples * p["train_repeat"]
            if not debug:
                random.shuffle(self.list_samples)
        else:
            self.list_samples = self.list_samples * p["val_repeat"]
        assert len(self.list_samples) > 0

    def __len__(self):
        return len(self.list_samples)

    # ---- music.py:56-92
    def get_samples(self, index, option="dc"):
        infos = [self.list_samples[index]]
        sound_cls = self.list_samples[index][5]
        if option == "dc":
            left = self.classes.copy()
            for _ in range(self.num_mix - 1):
                left.remove(sound_cls)          # (sic) raises ValueError for num_mix > 2, like the reference
                infos.append(random.choice(self.dict_samples[random.choice(left)]))
        elif option == "sc":
            for _ in range(self.num_mix - 1):
                infos.append(random.choice(self.dict_samples[sound_cls]))
        elif option == "sv":
            infos += [self.list_samples[index]] * (self.num_mix - 1)
        elif option == "random":
            for _ in range(self.num_mix - 1):
                infos.append(self.list_samples[random.randint(0, len(self.list_samples) - 1)])
        elif option == "vis1":
            infos = [random.choice(self.dict_samples["cello"])]
            for _ in range(self.num_mix - 1):
                infos.append(random.choice(self.dict_samples["flute"]))
        assert self.num_mix == len(infos)
        return infos

    def choose(self, index):
        """The strategy draw of music.py:283-289 (each elif draws a fresh random number, like the reference)."""
        if self.random_sample:
            return self.get_samples(index, "random")
        if self.vis_data:
            return self.get_samples(index, self.vis_data)
        if random.random() < self.rate_dc:
            return self.get_samples(index, "dc")
        if random.random() < self.rate_dc + self.rate_sc:
            return self.get_samples(index, "sc")
        if random.random() < self.rate_dc + self.rate_sc + self.rate_sv:
            return self.get_samples(index, "sv")
        raise UnboundLocalError("no sampling strategy drawn (rate_dc + rate_sc + rate_sv < 1): the reference fails here too")

    # ---- base.py:149-172
    def _load_audio_file(self, path, center_t):
        assert path.endswith(".wav")
        return read_wav_segment(path, self.audRate, center_t - self.margin - self.audSec / 2, self.margin * 2 + self.audSec)

    def _load_audio(self, path, center_t):
        audio = np.zeros(self.audLen, dtype=np.float32)
        raw, _ = self._load_audio_file(path, center_t)
        center_idx = int((self.margin + self.audSec / 2) * self.audRate)
        start = max(0, center_idx - self.audLen // 2)
        end = min(len(raw), center_idx + self.audLen // 2 + self.audLen % 2)
        audio[:max(end - start, 0)] = raw[start:end]
        if self.split == "train":
            audio *= random.random() + 0.5
        np.clip(audio, -1.0, 1.0, out=audio)
        return audio

    # ---- music.py:96-130
    def get_audios(self, infos):
        audios, center_times = [], []
        for n in range(self.num_mix):
            apath, _, num_f, fps, a_len, _ = infos[n]
            act_len = min(int(num_f) / float(fps), float(a_len))
            for j in range(10):
                end = act_len - self.margin - self.audSec / 2
                start = self.margin + self.audSec / 2
                if start > end:
                    end = act_len - self.audSec / 2
                    start = self.audSec / 2
                t = random.uniform(0 + start, end)
                aud = self._load_audio(apath, t)
                if self.split == "train":
                    silent = bool(np.all(aud == 0))
                else:
                    silent = ((np.abs(aud) < 0.001).sum() / self.audLen) > self.max_silent
                if not silent or j == 9:
                    if silent:
                        print(f"Load {apath} failed.")
                    center_times.append(t)
                    audios.append(aud / self.num_mix)
                    break
        return audios, np.asarray(audios).sum(axis=0), center_times

    # ---- music.py:132-156
    def frame_paths(self, info, center_t):
        _, fpath, _, fps, _, _ = info
        center_idx = round(center_t * float(fps))
        if self.one_frame:
            shift = random.randint(int(-1 * self.stride_frames), int(1 * self.stride_frames))
            return [os.path.join(fpath, "{:06d}.jpg".format(center_idx + shift))], center_idx
        return [os.path.join(fpath, "{:06d}.jpg".format(center_idx + (i - self.num_frames // 2) * self.stride_frames))
                for i in range(self.num_frames)], center_idx

    @staticmethod
    def _open_frames(paths):
        from PIL import Image
        return [Image.open(p).convert("RGB") for p in paths]

    def _load_frames(self, paths):
        return self.vid_transform(self._open_frames(paths))

    def _load_raw_frames(self, paths):
        """The clip as decoded, with the draws VideoTransform would make for it, in its order -> (uint8 [bytes]: the frames
        [H,W,3] back to back, int32 [T,2] their (H, W), crop (i, j) | None, flip)."""
        arrays = [np.asarray(f, dtype=np.uint8) for f in self._open_frames(paths)]
        H, W = arrays[0].shape[:2]
        crop, flip = draw_crop_flip(*self.vid_transform.resized_size(W, H), self.imgSize, self.vid_transform.train)
        pixels = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrays]))
        return pixels, torch.tensor([a.shape[:2] for a in arrays], dtype=torch.int32), crop, flip

    def _load_jpeg_frames(self, paths):
        """The clip as it lies in its files, with the same draws in the same order -> (uint8 [bytes]: the files back to back,
        int64 [T] their lengths, int32 [T,2] the frames' (H, W), crop, flip, [(t, uint8 pixels [H*W*3])] for the files the GPU
        decoder refuses (jpeg.probe and jpeg.probe_scans), decoded here as ``_open_frames`` decodes them)."""
        from . import jpeg
        files, shapes, fallback = [], [], []
        for t, path in enumerate(paths):
            with open(path, "rb") as f:
                files.append(f.read())
            try:
                try:
                    info = jpeg.probe(files[-1])
                except jpeg.Unsupported:
                    info = jpeg.probe_scans(files[-1])       # a progressive file: to_device decodes those on the GPU too
                shapes.append((info.H, info.W))
            except jpeg.Unsupported:
                a = np.asarray(self._open_frames([path])[0], dtype=np.uint8)
                shapes.append(a.shape[:2])
                fallback.append((t, torch.from_numpy(a.reshape(-1).copy())))
        H, W = shapes[0]
        crop, flip = draw_crop_flip(*self.vid_transform.resized_size(W, H), self.imgSize, self.vid_transform.train)
        data = torch.from_numpy(np.frombuffer(b"".join(files), dtype=np.uint8).copy())
        return (data, torch.tensor([len(f) for f in files], dtype=torch.int64), torch.tensor(shapes, dtype=torch.int32), crop, flip,
                fallback)

    def _load_raw(self, paths):
        """One clip of a raw item, in one form for both kinds: (data, lengths | None, shapes, crop, flip, fallback)."""
        if self.jpeg_bytes:
            return self._load_jpeg_frames(paths)
        pixels, shapes, crop, flip = self._load_raw_frames(paths)
        return pixels, None, shapes, crop, flip, []

    def get_frames(self, infos, center_times):
        frames, shifts = [], []
        for n in range(self.num_mix):
            paths, center_idx = self.frame_paths(infos[n], center_times[n])
            shifts.append(center_times[n] - center_idx / float(infos[n][3]))
            frames.append(self._load_raw(paths) if self.raw_frames else self._load_frames(paths))
        return frames, shifts

    # ---- music.py:240-252
    def get_ids_labels(self, infos, index, center_times):
        cls = [self.class_int_map[i[5]] for i in infos]
        ids = [os.path.basename(i[0]).split(".")[0][:4] for i in infos]
        name = (str(index) + "_cls" + "_".join(str(c) for c in cls) + "_ids" + "_".join(ids) + "_ct" +
                "_".join(str(round(t)) for t in center_times))
        return name, torch.tensor(cls)

    def __getitem__(self, index):
        random.seed(index)
        infos = self.choose(index)
        audios, mixture, center_times = self.get_audios(infos)
        frames, _ = self.get_frames(infos, center_times)
        name, cls = self.get_ids_labels(infos, index, center_times)
        item = {"infos": infos, "audios": [torch.from_numpy(a) for a in audios], "audio_mix": torch.from_numpy(mixture),
                "id": name, "class": cls}
        if not self.raw_frames:
            item["frames"] = frames
            return item
        # per source: the decoded pixels, the frames' shapes and the clip's draws (RAW_KEYS); no "frames" until to_device
        item.update({"frames_jpeg" if self.jpeg_bytes else "frames_u8": [f[0] for f in frames], "frame_shapes": [f[2] for f in frames],
                     "frame_crops": [f[3] for f in frames], "frame_flips": [f[4] for f in frames],
                     "imgSize": self.imgSize, "split": self.split})
        if self.jpeg_bytes:
            item.update({"frame_bytes": [f[1] for f in frames], "frames_fallback": [f[5] for f in frames]})
        return item


# ------------------------------------------------------------------------------------------ hand-off
def _stack(ts):
    # No pinning here: with workers > 0 this runs in fork()ed children of a process that may already have
    # initialised HIP, where hipHostMalloc is unusable — and a tensor returned through the worker queue is copied
    # into shared memory anyway.  The parent pins (DataLoader(pin_memory=True): its pin thread runs in the main process).
    return torch.stack(ts, 0)


def collate(samples):
    """default_collate's layout for this dict (lists of per-source tensors stay lists; `infos` transposed like
    default_collate does for nested lists of strings).  GPU-free: safe in forked workers.
    A batch of raw items (MUSICMixDataset(raw_frames=True)) has, instead of "frames", with N sources, B items, T frames:
      "frames_u8"     uint8 [bytes]: every frame [H,W,3] back to back, in the order source, item, time;
      "frame_shapes"  int32 [N,B,T,2]: (H, W) of every frame;
      "frame_crops"   int32 [N,B,2]: the clips' drawn corners (i, j), or None in the validation form (every frame its centre);
      "frame_flips"   bool [N,B];
      "imgSize" int and "split" str, as the dataset has them.
    A batch of MUSICMixDataset(raw_frames=True, jpeg_bytes=True) has, instead of "frames_u8":
      "frames_jpeg"    uint8 [bytes]: every frame's file back to back, in the same order;
      "frame_bytes"    int64 [N,B,T]: the files' lengths;
      "fallback_index" int64 [k] and "fallback_u8" uint8 [bytes]: the frames (n * B + b) * T + t whose files the GPU decoder
                       refuses, ascending, and their pixels [H,W,3] as the worker decoded them, back to back.
    ``to_device`` turns these into "frames"."""
    N = len(samples[0]["audios"])
    out = {"audios": [_stack([s["audios"][n] for s in samples]) for n in range(N)],
           "audio_mix": _stack([s["audio_mix"] for s in samples]),
           "id": [s["id"] for s in samples], "class": torch.stack([s["class"] for s in samples], 0),
           "infos": [[[s["infos"][n][k] for s in samples] for k in range(len(samples[0]["infos"][n]))] for n in range(N)]}
    if "frames_u8" not in samples[0] and "frames_jpeg" not in samples[0]:
        out["frames"] = [_stack([s["frames"][n] for s in samples]) for n in range(N)]
        return out
    if "frames_jpeg" in samples[0]:
        out["frames_jpeg"] = torch.cat([s["frames_jpeg"][n] for n in range(N) for s in samples])
        out["frame_bytes"] = torch.stack([torch.stack([s["frame_bytes"][n] for s in samples]) for n in range(N)])
        B, T = len(samples), out["frame_bytes"].shape[2]
        late = [((n * B + b) * T + t, px) for n in range(N) for b, s in enumerate(samples) for t, px in s["frames_fallback"][n]]
        out["fallback_index"] = torch.tensor([i for i, _ in late], dtype=torch.int64)
        out["fallback_u8"] = torch.cat([px for _, px in late]) if late else torch.zeros(0, dtype=torch.uint8)
    else:
        out["frames_u8"] = torch.cat([s["frames_u8"][n] for n in range(N) for s in samples])
    out["frame_shapes"] = torch.stack([torch.stack([s["frame_shapes"][n] for s in samples]) for n in range(N)])
    crops = [[s["frame_crops"][n] for s in samples] for n in range(N)]
    out["frame_crops"] = None if crops[0][0] is None else torch.tensor(crops, dtype=torch.int32)
    out["frame_flips"] = torch.tensor([[s["frame_flips"][n] for s in samples] for n in range(N)], dtype=torch.bool)
    out["imgSize"], out["split"] = samples[0]["imgSize"], samples[0]["split"]
    return out


def _decode_jpeg(batch, device):
    """The pixel buffer of a batch of files: decoded on the GPU (jpeg.decode), the workers' fallback pixels dropped into their
    slots -> uint8 [bytes] on the device, what "frames_u8" holds in a batch without jpeg_bytes."""
    from . import jpeg
    data, ends = batch["frames_jpeg"].numpy(), np.cumsum(batch["frame_bytes"].reshape(-1).numpy())
    files = [data[a:b].tobytes() for a, b in zip(np.concatenate([[0], ends[:-1]]), ends)]
    shapes = batch["frame_shapes"].reshape(-1, 2).tolist()
    decoded, at = {}, 0
    for i in batch["fallback_index"].tolist():
        n = shapes[i][0] * shapes[i][1] * 3
        decoded[i] = batch["fallback_u8"][at:at + n].numpy().reshape(shapes[i][0], shapes[i][1], 3)
        at += n
    pixels, got = jpeg.decode(files, device, decoded=decoded, progressive=True)
    if [list(s) for s in got] != shapes:
        raise ValueError("the frames' sizes changed between the workers' probe and the decode")
    return pixels


def _prepare_raw(batch, device):
    """The "frames" of a raw batch: one upload of the bytes, one launch for every source -> N tensors [B,3,T,S,S]."""
    from . import frames as F
    N, B, T, _ = batch["frame_shapes"].shape
    train, crops = batch["split"] == "train", batch["frame_crops"]
    per_clip = [None] * (N * B) if crops is None else [tuple(c) for c in crops.reshape(N * B, 2).tolist()]
    plan = F.plan_batch(batch["frame_shapes"].reshape(-1, 2).tolist(), batch["imgSize"], train=train,
                        crops=[c for c in per_clip for _ in range(T)],
                        flips=[f for f in batch["frame_flips"].reshape(-1).tolist() for _ in range(T)], layout=(N * B, T))
    if "frames_jpeg" in batch:
        pixels = _decode_jpeg(batch, device)
    else:
        pixels = batch["frames_u8"].to(device, non_blocking=True)
    out = F.prepare_batch(pixels, plan)
    return list(out.view(N, B, 3, T, plan.img_size, plan.img_size).unbind(0))


def to_device(batch, device):
    """Asynchronous H2D of the tensors of a collated batch (pinned source -> non_blocking copies on the current stream).  A raw
    batch (``collate``) uploads its bytes and gets its "frames" from the GPU (frames.prepare_batch), bit for bit what the
    workers' VideoTransform would have made of them."""
    mv = lambda t: t.to(device, non_blocking=True)      # noqa: E731
    out = dict(batch)
    out["audios"] = [mv(t) for t in batch["audios"]]
    out["frames"] = _prepare_raw(batch, device) if "frames_u8" in batch or "frames_jpeg" in batch else [mv(t) for t in batch["frames"]]
    out["audio_mix"] = mv(batch["audio_mix"])
    return out


def make_loader(csv_paths, args, split, batch_size, shuffle, workers=0, **kw):
    """ConcatDataset of the lists + DataLoader (main.py:633-659); batches are pinned by the parent's pin thread."""
    sets = [MUSICMixDataset(pth, vars(args), split=split, **kw) for pth in csv_paths]
    return torch.utils.data.DataLoader(torch.utils.data.ConcatDataset(sets), batch_size=batch_size, shuffle=shuffle,
                                       num_workers=workers, drop_last=False, collate_fn=collate,
                                       pin_memory=torch.cuda.is_available())
