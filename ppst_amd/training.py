"""The training loop around the HIP train step: what /root/reference/train.py:24-60 does
with util/iter_counter.py (image-count schedule, iter.txt resume), data/CelebAMask_dataset.py (image + label map ->
{'real_A', 'mask_A' one-hot}) and optimizers/ppst_optimizer.py -- plus optimiser-state checkpointing, which the
reference lacks (it restarts Adam from zero moments on resume).

Host logic only; every arithmetic step is in ppst_amd/train.py / train_g.py (HIP kernels).  Out of scope as in the
survey: visdom / HTML visualiser, the argparse option system, the tmux launcher.
"""
import os
import random
import time

import numpy as np
import torch

from . import glue, ops


class IterationCounter:
    """util/iter_counter.py:7-92: progress is counted in IMAGES; saving / evaluation / printing fire when the image
    count crosses a multiple of their period within one batch; ``iter.txt`` holds the count at the last save."""

    def __init__(self, opt):
        self.opt = opt
        self.iter_record_path = os.path.join(opt.checkpoints_dir, opt.name, "iter.txt")
        self.batch_size = opt.batch_size * (2 if "unaligned" in getattr(opt, "dataset_mode", "") else 1)
        self.time_measurements = {}
        self.steps_so_far = 0
        resume = getattr(opt, "resume_iter", "latest")
        cont = getattr(opt, "isTrain", True) and getattr(opt, "continue_train", False)
        if cont and resume == "latest" and getattr(opt, "pretrained_name", None) is None:
            try:
                self.steps_so_far = int(np.loadtxt(self.iter_record_path, delimiter=",", dtype=int))
                print("Resuming from iteration %d" % self.steps_so_far)
            except Exception:
                print("Could not load iteration record at %s. Starting from beginning." % self.iter_record_path)
        elif cont and str(resume).replace("k", "").isnumeric():
            steps = int(str(resume).replace("k", ""))
            self.steps_so_far = steps * 1000 if "k" in str(resume) else steps

    def record_one_iteration(self, write=True):
        """``write``: only rank 0 writes iter.txt (the reference calls this inside its ``local_rank == 0`` block, train.py:33-56;
        here every rank advances its count, one writes) -- through a temporary file, so a reader never sees a truncated record."""
        if write and self.needs_saving():
            os.makedirs(os.path.dirname(self.iter_record_path), exist_ok=True)
            tmp = self.iter_record_path + ".tmp%d" % os.getpid()
            np.savetxt(tmp, [self.steps_so_far], delimiter=",", fmt="%d")
            os.replace(tmp, self.iter_record_path)
        self.steps_so_far += self.batch_size

    def needs_saving(self):
        return (self.steps_so_far % self.opt.save_freq) < self.batch_size

    def needs_evaluation(self):
        return self.steps_so_far >= self.opt.evaluation_freq and (self.steps_so_far % self.opt.evaluation_freq) < self.batch_size

    def needs_printing(self):
        return (self.steps_so_far % self.opt.print_freq) < self.batch_size

    def completed_training(self):
        return self.steps_so_far >= self.opt.total_nimgs

    class _Timer:
        def __init__(self, name, parent):
            self.name, self.parent = name, parent

        def __enter__(self):
            self.t0 = time.time()

        def __exit__(self, *exc):
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            dt = (time.time() - self.t0) / self.parent.batch_size
            tm = self.parent.time_measurements
            tm[self.name] = dt if self.name not in tm else tm[self.name] * 0.98 + dt * 0.02     # EMA 0.98 (:84-88)

    def time_measurement(self, name):
        return IterationCounter._Timer(name, self)


class MetricTracker:
    """util/metric_tracker.py:9-23: exponential moving average (0.98) of the reported losses."""

    def __init__(self):
        self.metrics = {}

    def update_metrics(self, d, smoothe=True):
        for k, v in d.items():
            v = float(v)
            self.metrics[k] = self.metrics[k] * 0.98 + v * 0.02 if (smoothe and k in self.metrics) else v

    def current_metrics(self):
        return dict(self.metrics)


class CelebAMaskDataset:
    """data/CelebAMask_dataset.py:20-60 + data/__init__.py's per-rank sharding: <dataroot>/images/*.jpg|png and
    <dataroot>/labels/<same stem>.png (integer label map {0, 1, 2}, g_mask.py's aggregation).  Images are decoded on the
    host, resized and normalised ON THE DEVICE with the Pillow-exact kernels (ppst_amd/imageio.py); label maps are turned into
    one-hot masks by the exact glue kernel (:54-60).  ``next()`` yields batches forever (ConfigurableDataLoader,
    data/__init__.py:131-149), shuffled per epoch with a DistributedSampler-style split: sample k of an epoch's permutation
    belongs to rank k mod world; ``batch_size`` is the PER-RANK batch (the reference's ``opt.batch_size / opt.num_gpus``,
    data/__init__.py:116).

    The defaults are the launcher's TRAINING transform (preprocess="resize" + RandomHorizontalFlip, CelebA_launcher.py:17-18,
    base_dataset.py:130-132); the evaluators' transform (short side scaled, no flip) is passed explicitly at its call sites.
    ``preprocess``: "resize" = the launcher's training transform (square ``load_size``, CelebA_launcher.py:17-18);
    "scale_shortside" = the evaluators' transform.  ``flip``: RandomHorizontalFlip as in the reference's training transform
    (``no_flip`` is not set there).  Two stated deviations: (1) the reference builds the image and the label transform
    separately, so its two RandomHorizontalFlips draw independently and image / mask can end up mirrored against each other
    (base_dataset.py:130-132, CelebAMask_dataset.py:17-18); here ONE draw flips both.  (2) the reference resizes the 'L' label
    image with its BICUBIC transform and then compares ``mask_np == i``; at the dataset's native 512 that is the identity, off
    size it invents label values -- here labels are resized NEAREST.  The next batch is decoded on a worker thread while the
    current step runs (the reference: DataLoader workers).  ``decode="device"``: the worker thread only reads the files and
    parses their headers; ``next()`` decodes the batch's JPEG files in one call of the HIP JPEG decoder and its PNG files -- images
    and labels together -- in one call of the HIP PNG decoder (ops.jpeg_decode, ops.png_decode), the flip as their ``mirror`` -- the
    same batches, bit for bit.  A label file takes that path when it is a grey (colour type 0) PNG whose size already equals the
    preprocessed image's: it is mirrored with the image's draw and cast to int64 on the device.  Every other label file keeps the
    Pillow ``convert("L")`` + NEAREST path, and image files the decoders do not take go through Pillow as before."""

    def __init__(self, dataroot, size=512, batch_size=2, rank=0, world=1, device="cuda", seed=0, preprocess="resize",
                 flip=True, prefetch=True, decode="host"):
        assert preprocess in ("resize", "scale_shortside")
        if decode not in ("host", "device"):
            raise ValueError("decoder must be one of ('host', 'device'), not %r" % (decode,))
        self.decode = decode
        self.size, self.batch_size, self.rank, self.world, self.device = size, batch_size, rank, world, device
        self.preprocess, self.flip, self.prefetch = preprocess, flip, prefetch
        img_dir, lab_dir = os.path.join(dataroot, "images"), os.path.join(dataroot, "labels")
        exts = (".jpg", ".jpeg", ".png")
        names = sorted(f for f in os.listdir(img_dir) if f.lower().endswith(exts))
        self.pairs = [(os.path.join(img_dir, f), os.path.join(lab_dir, os.path.splitext(f)[0] + ".png")) for f in names]
        if not self.pairs:
            raise RuntimeError("no images under %s" % img_dir)
        self.epoch, self.pos, self.rng = 0, 0, random.Random(seed)
        self._order = self._epoch_order()
        self._next = None

    def __len__(self):
        return len(self.pairs)

    def _epoch_order(self):
        g = random.Random(1000003 * self.epoch + 17)        # same permutation on every rank (DistributedSampler.set_epoch)
        order = list(range(len(self.pairs)))
        g.shuffle(order)
        return order[self.rank::self.world] or order[:1]

    def _out_size(self, W, H):
        """(W, H) of the preprocessed image of a W x H file"""
        from . import imageio
        if self.preprocess == "resize":
            return imageio.make_power_2_size(self.size, self.size)
        return imageio.make_power_2_size(*imageio.scale_shortside_size(W, H, self.size))

    def _decode(self, idx):
        """host side: file -> (uint8 HWC image, PIL 'L' label), optionally mirrored together.  With the device decoder a JPEG or PNG
        file it takes stays bytes here: the image is then (bytes, mirror flag, path, what its codec parsed: an entry of the decode
        call's ``parsed``), and so is the label where it is a grey PNG of the preprocessed image's size.  Which codec takes a
        file: ops.codec_for."""
        from PIL import Image
        ip, lp = self.pairs[idx]
        try:
            blob, lblob = None, None
            if self.decode == "device" and ops.codec_for(ip) is not None:
                with open(ip, "rb") as f:
                    blob = f.read()
                rc, desc, head = ops.codec_for(ip).parse(blob)
                wh = (head.W, head.H)
                if rc != 0:
                    blob = None
            img = np.asarray(Image.open(ip).convert("RGB")) if blob is None else None
            if self.decode == "device":
                with open(lp, "rb") as f:
                    lblob = f.read()
                rc, ldesc, d = ops.PNG.parse(lblob)
                if rc != 0 or d.colour != 0 or (d.W, d.H) != self._out_size(*(wh if blob is not None else (img.shape[1], img.shape[0]))):
                    lblob = None
            lab = Image.open(lp).convert("L") if lblob is None else None
        except OSError as err:                                   # CelebAMask_dataset.py:33-38: retry a random index
            print(err)
            return self._decode(self.rng.randrange(len(self.pairs)))
        flip = bool(self.flip and self.rng.random() < 0.5)
        if flip:
            img = np.ascontiguousarray(img[:, ::-1]) if img is not None else None
            lab = lab.transpose(Image.FLIP_LEFT_RIGHT) if lab is not None else None
        return (img if blob is None else (blob, flip, ip, desc)), (lab if lblob is None else (lblob, flip, lp, ldesc))

    def _decode_on_device(self, batch):
        """[(image | (bytes, flip, path, descriptor), label)] -> the same with every image a uint8 HWC array or device tensor: one
        batched call.  A file that comes back with a status goes to Pillow; if Pillow raises OSError too, the sample is replaced by
        a random index as in ``_decode`` (that draw is then made on the consumer's thread: the order of draws, and so the batches
        that follow, differ from ``decode="host"`` from such a file on -- with sound files the two give the same batches)."""
        from PIL import Image
        todo = {}                                                # codec's name -> [(sample, 0: image / 1: label)]; labels are PNG files
        for n, pair in enumerate(batch):
            for k in (0, 1):
                if isinstance(pair[k], tuple):
                    todo.setdefault((ops.PNG if k else ops.codec_for(pair[k][2])).name, []).append((n, k))
        if not todo:
            return batch
        done = {}                                                # (sample, 0: image / 1: label) -> (view, status)
        for codec in ops.CODECS:
            keys = todo.get(codec.name)
            if not keys:
                continue
            items = [batch[n][k] for n, k in keys]
            flags = dict(codec.rgb)                              # images come out RGB, labels as the one channel they are
            if any(k for _, k in keys):
                flags["expand_grey"] = [k == 0 for _, k in keys]
            views, status = codec.decode([it[0] for it in items], mirror=[it[1] for it in items], device=self.device,
                                         parsed=[it[3] for it in items], **flags)
            done.update(zip(keys, zip(views, status.cpu().tolist())))
        batch = [list(pair) for pair in batch]
        for (n, k), (v, st) in sorted(done.items()):
            if batch[n] is None:
                continue
            _, flip, path, _ = batch[n][k]
            if st != 0:                                          # damaged data: what the host decoder makes of it
                try:
                    v = Image.open(path).convert("L" if k else "RGB")
                    v = (v.transpose(Image.FLIP_LEFT_RIGHT) if flip else v) if k else np.asarray(v)
                except OSError as err:                           # CelebAMask_dataset.py:33-38: retry a random index
                    print(err)
                    batch[n] = None
                    continue
                v = np.ascontiguousarray(v[:, ::-1]) if (flip and not k) else v
            batch[n][k] = v[:, :, 0] if (k and isinstance(v, torch.Tensor)) else v
        return [tuple(pair) if pair is not None else self._decode_on_device([self._decode(self.rng.randrange(len(self.pairs)))])[0]
                for pair in batch]

    def _to_device(self, img, lab):
        from PIL import Image
        from . import imageio
        fn = imageio.preprocess_resize if self.preprocess == "resize" else imageio.preprocess
        img = img if isinstance(img, torch.Tensor) else torch.from_numpy(img).to(self.device)
        x = fn(img[None], self.size)[0]
        H, W = x.shape[1], x.shape[2]
        if isinstance(lab, torch.Tensor):                        # decoded on the device: already (H, W), already mirrored
            assert tuple(lab.shape) == (H, W), (tuple(lab.shape), H, W)
            lab = lab.to(torch.int64)
        else:
            lab = torch.from_numpy(np.asarray(lab.resize((W, H), Image.NEAREST)).astype(np.int64))
        return x, lab

    def _load(self, idx):
        return self._to_device(*self._decode_on_device([self._decode(idx)])[0])

    def _decode_batch(self):
        out = []
        while len(out) < self.batch_size:
            if self.pos >= len(self._order):
                self.epoch, self.pos = self.epoch + 1, 0
                self._order = self._epoch_order()
            out.append(self._decode(self._order[self.pos]))
            self.pos += 1
        return out

    def __iter__(self):
        return self

    def __next__(self):
        if self.prefetch:
            import threading
            if self._next is None:
                cur = self._decode_batch()
            else:
                th, box = self._next
                th.join()
                if "err" in box:
                    raise box["err"]
                cur = box["batch"]
            box = {}

            def work():
                try:
                    box["batch"] = self._decode_batch()
                except Exception as e:       # surfaced by the consumer's next call
                    box["err"] = e
            th = threading.Thread(target=work, daemon=True)
            th.start()
            self._next = (th, box)
        else:
            cur = self._decode_batch()
        xs, labs = zip(*(self._to_device(img, lab) for img, lab in self._decode_on_device(cur)))
        labels = torch.stack([lab.to(self.device) for lab in labs])
        return {"real_A": torch.stack(xs).contiguous(), "mask_A": glue.one_hot_mask(labels)}


class SyntheticMaskDataset:
    """Stand-in with the same interface (no dataset ships with the repo): smooth synthetic portraits + block label maps."""

    def __init__(self, size=512, batch_size=2, rank=0, device="cuda", seed=0):
        self.size, self.batch_size, self.rank, self.device, self.k = size, batch_size, rank, device, seed

    def __iter__(self):
        return self

    def __next__(self):
        from . import weights as W
        self.k += 1
        real = W.synthetic_images(1000 * self.rank + self.k, self.batch_size, self.size).to(self.device)
        g = torch.Generator().manual_seed(7919 * self.rank + self.k)
        s = self.size // 16
        lab = torch.randint(0, 3, (self.batch_size, s, s), generator=g).repeat_interleave(16, 1).repeat_interleave(16, 2)
        return {"real_A": real, "mask_A": glue.one_hot_mask(lab.to(self.device))}


# ---------------------------------------------------------------------------------------------- optimiser state
def save_optimizer_state(optimizer, path):
    """Adam moments + step counts of all four networks and the D / G alternation state.  The reference saves the model
    only (base_model.py:33-41) and resumes with zero moments; this makes a resumed run continue the same trajectory."""
    st = {"train_mode_counter": optimizer.train_mode_counter}
    for k, f in optimizer.gen.owners().items():
        st[k] = {"m": f.m.detach().cpu(), "v": f.v.detach().cpu(), "step": f.step_count}
        if k == "D":
            st[k]["iter_counter"] = f.iter_counter
    torch.save(st, path)
    return path


def load_optimizer_state(optimizer, path):
    st = torch.load(path, map_location="cpu", weights_only=True)        # nested dicts of tensors / ints only: nothing is executed
    optimizer.train_mode_counter = int(st["train_mode_counter"])
    for k, f in optimizer.gen.owners().items():
        if k == "D" and "D" not in st:          # (a file written for a model without a discriminator)
            continue
        if f.m.numel() != st[k]["m"].numel():
            raise ValueError("optimizer state of %s has %d entries, the network has %d" % (k, st[k]["m"].numel(), f.m.numel()))
        f.m.copy_(st[k]["m"]); f.v.copy_(st[k]["v"]); f.step_count = int(st[k]["step"])
        if k == "D":
            f.iter_counter = int(st[k]["iter_counter"])
    return optimizer


class HeldOutEvaluator:
    """Reconstruction quality on a FIXED set of held-out images, for ``train_loop(evaluator=...)`` -- the place where the
    reference's train.py runs its evaluators (train.py:52-56).  ``__call__(model, steps)`` returns the means of
    ``evaluation.evaluate_reconstruction`` over the images as {name: float}, appends one line to ``log_path`` (None: the loop
    resolves it to <checkpoints_dir>/<name>/eval_log.txt) and keeps (steps, result) in ``.history``.  It issues no collective:
    only rank 0 calls it, the other ranks simply reach their next all-reduce first.
    ``swaps=True`` (at least two images): it also runs ``evaluation.simple_swap`` of image i with style (i + 1) mod N under
    ``no_grad`` and adds ``swap_content_ssim`` (``evaluation.content_preservation``), ``swap_style_w1`` / ``swap_style_swd`` /
    ``swap_style_delta_e`` (``evaluation.style_fidelity``'s w1_rgb, swd and delta_e: means over the pairs and the non-empty
    regions) and ``identity_style_w1``, the same w1 between each content and its style BEFORE the swap: what no transfer at all
    scores on these images.  ``labels`` (integer (N, H, W) maps or one-hot masks of the images, three regions): the distances are
    taken per region, and the three style numbers are also reported per region as ``..._r0``, ``_r1``, ``_r2``.
    ``set_baseline(method)`` (with ``swaps=True``; the constructor's parameter list is pinned, so the choice is made on the
    object: ``HeldOutEvaluator(x, swaps=True).set_baseline("hist")``): "hist", "mkl" or "reinhard" -- the same pairs also go
    through ``evaluation.baseline_swap`` with that method (no feather, no guided filter) and are scored the same way as
    ``baseline_content_ssim``, ``baseline_style_w1``, ``baseline_style_swd`` and ``baseline_style_delta_e`` (per region with
    labels): what a classical per-region colour transfer scores where the model scores ``swap_...``.  None adds nothing."""

    STYLE_KEYS = (("swap_style_w1", "w1_rgb"), ("swap_style_swd", "swd"), ("swap_style_delta_e", "delta_e"))

    baseline = None

    def __init__(self, images, log_path=None, batch=8, swaps=False, labels=None):
        if swaps and images.shape[0] < 2:
            raise ValueError("HeldOutEvaluator(swaps=True) needs at least two images, got %d" % images.shape[0])
        self.images, self.log_path, self.batch, self.swaps, self.labels = images, log_path, batch, swaps, labels
        self.history = []

    def set_baseline(self, method):
        """choose the classical baseline reported beside the swap numbers (None: none); returns the evaluator"""
        from .metrics import TRANSFER_METHODS
        if method is not None and method not in TRANSFER_METHODS:
            raise ValueError("HeldOutEvaluator.set_baseline takes None or one of %s, got %r" % (TRANSFER_METHODS, method))
        if method is not None and not self.swaps:
            raise ValueError("HeldOutEvaluator.set_baseline needs swaps=True: the baseline runs on the swap pairs")
        self.baseline = method
        return self

    def evaluate_swaps(self, model):
        """the swap numbers of ``swaps=True`` as {name: float}"""
        from . import evaluation
        N = self.images.shape[0]
        style_of = [(i + 1) % N for i in range(N)]
        styles = self.images[style_of]
        lab = self.labels
        lab_s = None if lab is None else lab[style_of]
        with torch.no_grad():
            out = torch.cat([evaluation.simple_swap(model, self.images[i:i + self.batch], styles[i:i + self.batch])[1.0]
                             for i in range(0, N, self.batch)], 0)
        nanmean = lambda t: float(t[~t.isnan()].mean().item())
        res = {"swap_content_ssim": float(evaluation.content_preservation(self.images, out).double().mean().item())}
        fid = evaluation.style_fidelity(styles, out, lab_s, lab)
        for key, name in self.STYLE_KEYS:
            res[key] = nanmean(fid[name])
            if lab is not None:
                for r in range(fid[name].shape[1]):
                    res["%s_r%d" % (key, r)] = nanmean(fid[name][:, r])
        res["identity_style_w1"] = nanmean(evaluation.style_fidelity(styles, self.images, lab_s, lab)["w1_rgb"])
        if self.baseline is not None:
            base = evaluation.baseline_swap(self.images, styles, lab, lab_s, method=self.baseline)
            res["baseline_content_ssim"] = float(evaluation.content_preservation(self.images, base).double().mean().item())
            fid = evaluation.style_fidelity(styles, base, lab_s, lab)
            for key, name in self.STYLE_KEYS:
                key = key.replace("swap_", "baseline_")
                res[key] = nanmean(fid[name])
                if lab is not None:
                    for r in range(fid[name].shape[1]):
                        res["%s_r%d" % (key, r)] = nanmean(fid[name][:, r])
        return res

    @staticmethod
    def format(steps, result):
        return "(eval iters: %d) %s" % (steps, " ".join("%s: %.5f" % kv for kv in sorted(result.items())))

    def __call__(self, model, steps):
        from . import evaluation
        per_image = evaluation.evaluate_reconstruction(model, self.images, batch=self.batch)
        result = {k: float(v.double().mean().item()) for k, v in per_image.items()}
        if self.swaps:
            result.update(self.evaluate_swaps(model))
        self.history.append((int(steps), result))
        if self.log_path is not None:
            os.makedirs(os.path.dirname(os.path.abspath(self.log_path)), exist_ok=True)
            with open(self.log_path, "a") as f:
                f.write(self.format(steps, result) + "\n")
        return result


def train_loop(opt, model, dataset, optimizer, iter_counter=None, log=print, max_iterations=None, evaluator=None):
    """train.py:24-60: while not done: batch -> train_one_step (D / G alternation) -> EMA metrics -> rank 0 prints / saves
    (model checkpoint in the reference's layout + optimiser state + iter.txt).  Returns the metric tracker.
    ``evaluator``: a callable (model, steps) -> {name: number}, e.g. ``HeldOutEvaluator``; rank 0 calls it where
    ``iter_counter.needs_evaluation()`` fires (train.py:52-56) and prints its line through ``log``.  None (the default): nothing
    is evaluated and ``opt.evaluation_freq`` is never read."""
    iter_counter = iter_counter or IterationCounter(opt)
    if evaluator is not None and getattr(evaluator, "log_path", "") is None:
        evaluator.log_path = os.path.join(opt.checkpoints_dir, opt.name, "eval_log.txt")
    tracker = MetricTracker()
    rank0 = getattr(opt, "local_rank", 0) == 0
    n = 0
    while not iter_counter.completed_training():
        with iter_counter.time_measurement("data"):
            cur = next(dataset)
        with iter_counter.time_measurement("train"):
            losses = optimizer.train_one_step(cur, iter_counter.steps_so_far)
            tracker.update_metrics(losses, smoothe=True)
        if rank0:
            if iter_counter.needs_printing():
                tm = iter_counter.time_measurements
                log("(iters: %d) %s | %s" % (iter_counter.steps_so_far, " ".join("%s: %.3f" % kv for kv in tm.items()),
                                              " ".join("%s: %.3f" % kv for kv in sorted(tracker.current_metrics().items()))))
            if evaluator is not None and iter_counter.needs_evaluation():
                result = evaluator(model, iter_counter.steps_so_far)
                log(HeldOutEvaluator.format(iter_counter.steps_so_far, result))
            if iter_counter.needs_saving():
                save_all(opt, optimizer, iter_counter.steps_so_far)
        n += 1
        if iter_counter.completed_training() or (max_iterations is not None and n >= max_iterations):
            break
        iter_counter.record_one_iteration(write=rank0)
    if rank0:
        save_all(opt, optimizer, iter_counter.steps_so_far)
        log("Training finished.")
    return tracker


def save_all(opt, optimizer, steps):
    path = optimizer.save(steps)
    save_optimizer_state(optimizer, os.path.join(os.path.dirname(path), "latest_optimizer.pth"))
    return path
