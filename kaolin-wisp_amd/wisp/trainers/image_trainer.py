"""ImageTrainer: the trainer of the reference's image application (wisp/trainers/image_trainer.py:41-185) over this package's
BaseTrainer, and ImageTrainStep: the same optimisation - mean squared error of ImageNeuralField.rgb against sampled pixels, Adam with
the name-matched parameter groups - over one flat parameter buffer with the single-launch optimizer, replayable as a HIP graph.

image_hash.yaml trains with FusedAdam (= Adam), lr 1e-3, eps 1e-16, decoder weight decay 1e-6, grid lr x 500, a MultiStepLR
schedule, 4096 pixels per step, fp16 autocast.  Validation renders the whole image through render_image (one launch of
csrc/image_field.hip when the field is its shape) and takes the PSNR from the kernel's squared-error partials; the reference's
parquet / git / tensorboard logging stays out, as in the other trainers here."""
import logging as log
import os

import numpy as np
import torch
import torch.nn.functional as F

from wisp.trainers.base_trainer import BaseTrainer
from wisp.trainers.multiview_trainer import FlatParams


def _hip():
    import wisp._C as _C
    return _C


class _ItemLoader:
    """The DataLoader of base_trainer.py:197-203 for a dataset whose items are tuples of tensors that already live on the device:
    `batch_size` items per batch in a fresh random order every epoch, collated as torch's default collate does a tuple - every
    member stacked under a leading batch dimension (which ImageTrainer.step asserts to be 1 and squeezes again)."""

    def __init__(self, dataset, batch_size):
        self.dataset, self.batch_size = dataset, max(int(batch_size), 1)

    def __len__(self):
        return max(-(-len(self.dataset) // self.batch_size), 1)

    def __iter__(self):
        order = torch.randperm(len(self.dataset)).tolist()
        for i in range(0, len(order), self.batch_size):
            items = [self.dataset[j] for j in order[i:i + self.batch_size]]
            yield [torch.stack(member) if len(items) > 1 else member[0][None] for member in zip(*items)]


class ImageTrainer(BaseTrainer):
    """Events of step() in the reference's order (image_trainer.py:52-84): the batch dimension of 1 asserted and squeezed, the
    optimizer's zero_grad, the field and F.mse_loss under autocast, two metric read-backs, backward and optimizer step through the
    GradScaler when enable_amp, the scheduler."""

    def init_dataloader(self):
        self.train_data_loader = _ItemLoader(self.train_dataset, self.cfg.dataloader.batch_size)
        self.iterations_per_epoch = len(self.train_data_loader)

    def pre_training(self):
        super().pre_training()
        self.tracker.metrics.define_metric('rgb_loss', aggregation_type=float)

    def step(self, data):
        xy, target = (member.to(self.device) for member in data[:2])
        assert xy.shape[0] == 1, "ImageTrainer takes one item per batch (dataloader.batch_size = 1)"
        xy, target = xy.squeeze(0), target.squeeze(0)
        nef, metrics = self.pipeline.nef, self.tracker.metrics
        self.optimizer.zero_grad()
        # the reference enters torch.cuda.amp.autocast() here whatever enable_amp says; on a CPU device that is no autocast at all
        on_gpu = torch.device(self.device).type == 'cuda'
        with torch.autocast('cuda' if on_gpu else 'cpu', enabled=on_gpu):
            mse = F.mse_loss(nef.rgb(xy), target).mean()
            total = 0 + mse
        metrics.total_loss += total.item()                  # two read-backs per step, as the reference makes them
        metrics.rgb_loss += mse.item()
        if not self.cfg.enable_amp:
            total.backward()
            self.optimizer.step()
        else:
            self.scaler.scale(total).backward()
            self.scaler.step(self.optimizer)
            self.scaler.update()
        if self.cfg.scheduler:
            self.scheduler.step()

    def log_console(self):
        m = self.tracker.metrics
        log.info('EPOCH {}/{} | total loss: {:>.3E} | rgb loss: {:>.3E}'.format(
            self.epoch, self.max_epochs, m.average_metric('total_loss'), m.average_metric('rgb_loss')))

    def validate(self):
        """image_trainer.py:95-181 without its logging back-ends: render the image, PSNR against the ground truth, img_pred.png
        and img_gts.png into the tracker's log directory, return_dict[metric] = the best so far.  'ssim' (image_trainer.py:146-147)
        compares the float image with bank / 255 through wisp.ops.image.ssim on the GPU - one more render, the PSNR and the PNGs
        come from the same launch as without it; on any other device it is refused, as 'lpips' is everywhere."""
        from wisp.models.nefs.image_nef import fused_render_shape, render_image
        from wisp.ops.image import psnr, save_u8, ssim
        if 'lpips' in self.cfg.valid_metrics:
            raise NotImplementedError("valid_metrics: 'lpips' needs a package this project does not depend on (lpips); "
                                      "'psnr' and 'ssim' are provided")
        want_ssim = 'ssim' in self.cfg.valid_metrics
        if want_ssim and torch.device(self.device).type != 'cuda':
            raise NotImplementedError(f"valid_metrics: 'ssim' is computed on the GPU (wisp.ops.image.ssim has no host path); "
                                      f"this trainer's device is {self.device!r}")
        nef, ds = self.pipeline.nef, self.train_dataset
        nef.eval()
        h, w = ds.h, ds.w
        bank = ds.image_u8.to(self.device)
        want_psnr = 'psnr' in self.cfg.valid_metrics
        metrics_dict = {}
        if fused_render_shape(nef) is not None:
            # one launch: the u8 image and, per workgroup, the squared error against the u8 bank
            pred_u8, err = render_image(nef, h, w, out='u8', gts_u8=bank)
            if want_psnr:
                metrics_dict['psnr'] = 10 * np.log10(1.0 / (float(err) / (h * w * 3)))
            img = render_image(nef, h, w, out='f32').reshape(h, w, 3) if want_ssim else None
        else:
            img = render_image(nef, h, w, out='f32').reshape(h, w, 3)
            pred_u8 = (img * 255).byte()
            if want_psnr:
                metrics_dict['psnr'] = psnr(img, bank / 255.0)
        if want_ssim:
            metrics_dict['ssim'] = ssim(img, bank.reshape(h, w, 3) / 255.0)
        os.makedirs(self.tracker.log_dir, exist_ok=True)
        save_u8(os.path.join(self.tracker.log_dir, 'img_pred.png'), pred_u8.reshape(h, w, 3).cpu().numpy())
        # (the reference writes (gts * 255).byte() of gts = u8 / 255: fl(fl(v / 255) * 255) truncates back to v for all 256 values)
        save_u8(os.path.join(self.tracker.log_dir, 'img_gts.png'), bank.cpu().numpy())
        for name, value in metrics_dict.items():            # the best value so far is what train() returns
            self.return_dict[name] = max(self.return_dict.get(name, value), value)
            log.info(f"{name}: {value:.2f}")
            self.tracker.log_metric(f"validation/{name}", value, self.epoch)
        return metrics_dict

    def render_snapshot(self):
        return


class ImageTrainStep:
    """SDFTrainStep's pattern for the image field: parameters re-homed into one flat buffer (FlatParams), forward and backward
    through the modular 2-D lookup and decoder under autograd in fp32, loss = F.mse_loss, one fused optimizer launch that also
    zeroes the gradients.  `lr` is a plain attribute read at every step, so a MultiStepLR-style schedule is driven from outside
    (`set_schedule` installs image_hash.yaml's).  capture(batch_size) records forward + loss + backward as one HIP graph.
    fused=True takes forward + loss + backward through wisp_image_field_train_step (csrc/image_field_train.hip: two launches)
    whenever the field is that kernel's shape (_fused_field), and the modular launches otherwise; the default leaves every launch
    where it was."""

    def __init__(self, nef, lr=1e-3, eps=1e-16, weight_decay=0.0, grid_lr_weight=1.0, betas=(0.9, 0.999), optimizer='adam',
                 fused=False):
        self.nef = nef
        self.fused = bool(fused)
        self.flat = FlatParams(nef)
        self.lr, self.eps, self.weight_decay, self.grid_lr_weight, self.betas = lr, eps, weight_decay, grid_lr_weight, betas
        self.optimizer = str(optimizer).lower()
        if self.optimizer not in ('adamw', 'adam'):
            raise ValueError(f"optimizer must be 'adamw' or 'adam', got {optimizer!r}")
        self.opt_steps = 0
        self._milestones, self._gamma, self._base_lr = None, 1.0, lr

    def set_schedule(self, milestones, gamma):
        """torch.optim.lr_scheduler.MultiStepLR over this step's `lr`: after optimizer step number s, lr = base * gamma ** (number of
        milestones <= s).  As in torch, a milestone takes effect when the integer step count EQUALS it, so one that is not a whole
        number never does."""
        self._milestones, self._gamma, self._base_lr = sorted(milestones), gamma, self.lr

    def scheduled_lr(self):
        if self._milestones is None:
            return self.lr
        return self._base_lr * self._gamma ** sum(1 for m in self._milestones if m <= self.opt_steps and float(m).is_integer())

    def optimizer_step(self):
        C = _hip()
        self.opt_steps += 1
        f = self.flat
        groups = []
        # base_trainer.py:205-246: the decoder group names its weight decay, the others inherit the optimizer's default - the same value
        for g, lr in (("decoder", self.lr), ("grid", self.lr * self.grid_lr_weight), ("rest", self.lr)):
            a, b = f.ranges[g]
            if b > a:
                groups.append((a, b - a, lr, self.weight_decay, None))
        C.optim_step_groups(self.optimizer, f.data, f.grad, f.exp_avg, f.exp_avg_sq, groups, self.betas[0], self.betas[1], self.eps,
                            self.opt_steps, zero_grad=True)
        self.lr = self.scheduled_lr()

    def _fused_field(self):
        """What wisp_image_field_train_step needs, or None: only in a step built with fused=True, for the field shape of
        fused_render_shape (a 'cat' HashGrid without a BLAS, two f32 features per entry, at most 16 levels, the 3-octave embedder,
        one hidden relu Linear layer of at most 128 units with biases, 3 outputs), with f32, contiguous parameters and gradients
        on the GPU.  WISP_IMAGE_TRAIN_FUSED=0 keeps the modular launches (so does WISP_IMAGE_RENDER_FUSED=0, which makes
        fused_render_shape decline), and so does a batch of more than 2^22 pixels.  The shape checks are cached; what can change under a
        live trainer is looked at on every call (_fused_still_valid)."""
        if not self.fused:
            return None
        cached = getattr(self, "_fused_cache", None)
        if cached is not None:
            if cached and not self._fused_still_valid(cached):
                cached = self._fused_cache = None                  # re-derive below
            else:
                return cached or None
        self._fused_cache = False
        if os.environ.get("WISP_IMAGE_TRAIN_FUSED", "1") == "0":
            return None
        from wisp.models.nefs.image_nef import fused_render_shape
        shape = fused_render_shape(self.nef)
        if shape is None:
            return None
        grid, l1, lout = shape
        if not (1 <= l1.out_features <= 128 and lout.in_features == l1.out_features):
            return None
        prm = [grid.codebook.feats, l1.weight, l1.bias, lout.weight, lout.bias]
        if not all(q.is_cuda and q.dtype == torch.float32 and q.is_contiguous() and q.grad is not None and q.grad.is_contiguous()
                   and q.grad.dtype == torch.float32 and q.grad.is_cuda for q in prm):
            return None
        # the host-side description is kept (begin_idxes comes from a device tensor); the tensors are taken anew at every step.
        # rgb()'s default lod = num_lods - 1 blends the levels below it: the finest level is inert ('cat', hash_grid.py:226-229)
        host = dict(begin_idxes=grid.codebook.begin_idxes.tolist(), resolutions=grid.codebook.resolutions.reshape(-1).tolist(),
                    codebook_bitwidth=int(grid.codebook_bitwidth), active_lods=grid.num_lods - 1)
        self._fused_cache = dict(grid=grid, dec=self.nef.decoder, l1=l1, lout=lout, lods=grid.num_lods, prm=prm, host=host)
        return self._fused_cache

    def _fused_still_valid(self, c):
        nef = self.nef
        grid, dec = c["grid"], c["dec"]
        if not self.fused or getattr(nef, "grid", None) is not grid or getattr(nef, "decoder", None) is not dec \
                or grid.num_lods != c["lods"] or dec.layers[0] is not c["l1"] or dec.lout is not c["lout"]:
            return False
        now = [grid.codebook.feats, c["l1"].weight, c["l1"].bias, c["lout"].weight, c["lout"].bias]
        for q, was in zip(now, c["prm"]):
            g = q.grad
            if q is not was or g is None or g.dtype != torch.float32 or not g.is_contiguous() or not q.is_contiguous() \
                    or q.dtype != torch.float32:
                return False
        return True

    def _forward_backward(self, coords, rgb):
        fused = None
        if self.fused and coords.is_cuda and rgb.is_cuda and coords.ndim == 2 and rgb.ndim == 2 and 0 < coords.shape[0] <= (1 << 22) \
                and coords.shape[1] == 2 and tuple(rgb.shape) == (coords.shape[0], 3) and coords.dtype == rgb.dtype == torch.float32:
            fused = self._fused_field()
        if fused is not None:
            table, (w1, b1, w2, b2) = fused["prm"][0], fused["prm"][1:]
            fld = dict(fused["host"], codebook=table.detach(), w1=w1.detach(), b1=b1.detach(), w2=w2.detach(), b2=b2.detach())
            return _hip().image_field_train_step(coords, rgb, fld, table.grad, w1.grad, b1.grad, w2.grad, b2.grad)[0][0]
        loss = F.mse_loss(self.nef.rgb(coords), rgb)
        loss.backward()
        return loss.detach()

    def capture(self, batch_size):
        """Forward + loss + backward for a FIXED number of pixels as one HIP graph (see SDFTrainStep.capture): every shape in it
        is static, the optimizer launch stays outside.  step() replays it for batches of the captured size."""
        dev = self.flat.data.device
        if dev.type != 'cuda':
            raise RuntimeError("ImageTrainStep.capture needs the model on the GPU")
        self._g_coords = torch.zeros(batch_size, 2, dtype=torch.float32, device=dev)
        self._g_rgb = torch.zeros(batch_size, 3, dtype=torch.float32, device=dev)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                          # warm-up off the default stream (allocator, lazy set-up)
            for _ in range(3):
                self._forward_backward(self._g_coords, self._g_rgb)
        torch.cuda.current_stream().wait_stream(side)
        self.flat.grad.zero_()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):             # (on the warm-up stream: the ops' per-stream scratch lives there)
            self._g_loss = self._forward_backward(self._g_coords, self._g_rgb)
        self.flat.grad.zero_()
        self._graph = graph
        return self

    def static_inputs(self):
        if getattr(self, "_graph", None) is None:
            return None
        return self._g_coords, self._g_rgb

    def step(self, coords, rgb):
        """coords [B, 2], rgb [B, 3] on the field's device -> the loss (mean squared error) as a tensor."""
        graph = getattr(self, "_graph", None)
        if graph is not None and tuple(coords.shape) == tuple(self._g_coords.shape) and tuple(rgb.shape) == tuple(self._g_rgb.shape):
            if coords is not self._g_coords:
                self._g_coords.copy_(coords)
            if rgb is not self._g_rgb:
                self._g_rgb.copy_(rgb)
            graph.replay()
            self.optimizer_step()
            return self._g_loss.clone()
        loss = self._forward_backward(coords, rgb)
        self.optimizer_step()
        return loss
