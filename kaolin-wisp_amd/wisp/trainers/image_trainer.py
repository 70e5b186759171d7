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
        and img_gts.png into the tracker's log directory, return_dict['psnr'] = the best so far."""
        from wisp.models.nefs.image_nef import fused_render_shape, render_image
        from wisp.ops.image import psnr, save_u8
        for name in ('ssim', 'lpips'):
            if name in self.cfg.valid_metrics:
                raise NotImplementedError(f"valid_metrics: {name!r} needs a package this project does not depend on "
                                          f"({'scikit-image' if name == 'ssim' else 'lpips'}); only 'psnr' is provided")
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
        else:
            img = render_image(nef, h, w, out='f32').reshape(h, w, 3)
            pred_u8 = (img * 255).byte()
            if want_psnr:
                metrics_dict['psnr'] = psnr(img, bank / 255.0)
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
    (`set_schedule` installs image_hash.yaml's).  capture(batch_size) records forward + loss + backward as one HIP graph."""

    def __init__(self, nef, lr=1e-3, eps=1e-16, weight_decay=0.0, grid_lr_weight=1.0, betas=(0.9, 0.999), optimizer='adam'):
        self.nef = nef
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

    def _forward_backward(self, coords, rgb):
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
