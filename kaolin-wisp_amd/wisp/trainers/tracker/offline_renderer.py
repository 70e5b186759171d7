"""OfflineRenderer: non-interactive rendering of a pipeline from a look-at camera, with the shading modes and the slice helpers
of the NGLOD application (wisp/trainers/tracker/offline_renderer.py:23-330; constructor schema and attributes as there).

What differs from the reference:
  * `shadow=True` / `ao=True` raise NotImplementedError at construction: the reference's ambient-occlusion loop reads a name it
    never defines and its shadow pass needs a host-side Gaussian filter; neither is provided.
  * shading mode 'rb' on a field that answers 'rgb' and 'sdf' together (NeuralSDFTex) takes the colours from the field at the
    hit points (wisp.ops.sdf.sdf_query: one launch on an nglod-shaped field); the reference calls a `nef.rgb` no field defines.
  * render() sets `fused_normals` on a PackedSDFTracer for the duration of its traces (and restores what was there), so the normals are one launch (wisp_sdf_fd_gradient) instead of six
    field queries; sdf_slice / normal_slice handed a neural field (instead of a function) evaluate through
    wisp.ops.sdf.sdf_query / sdf_fd_gradient.  Handed a function they call it, as the reference does.
  * the model matrix goes to the rays' device instead of the literal 'cuda'.
"""
from __future__ import annotations

import time
from typing import Tuple

import numpy as np
import torch
import torch.nn.functional as F

from wisp.core import RenderBuffer, Rays
from wisp.ops.differential import finitediff_gradient
from wisp.ops.geometric import normalized_grid, normalized_slice
from wisp.ops.shaders import matcap_shader


def _look_at(f, t, height, width, mode='persp', fov=90.0, device='cuda'):
    """Rays of a camera at `f` looking at `t` with the world's y axis up: ([height * width, 3] origins, directions)."""
    origin = torch.tensor([float(v) for v in f], dtype=torch.float32, device=device)
    target = torch.tensor([float(v) for v in t], dtype=torch.float32, device=device)
    world_up = torch.tensor([0.0, 1.0, 0.0], device=device)
    view = F.normalize(target - origin, dim=0)
    right = F.normalize(torch.linalg.cross(view, world_up), dim=0)
    up = F.normalize(torch.linalg.cross(right, view), dim=0)
    return _generate_rays(origin, view, right, up, height, width, mode=mode, fov=fov, device=device)


def _generate_rays(camera_origin, camera_view, camera_right, camera_up, height, width, mode='persp', fov=90.0, device='cuda'):
    """Rays through the pixels of the image plane at unit distance in front of the camera: 'persp' - from the camera origin
    through the plane points; 'ortho' - from the plane points along the viewing direction.  ([height * width, 3], same)."""
    coord = normalized_grid(height, width, device=device)
    half = np.tan(np.radians(fov / 2))
    plane = camera_right * coord[..., 0, None] * half + camera_up * coord[..., 1, None] * half + camera_origin + camera_view
    plane = plane.reshape(-1, 3)
    if mode == 'ortho':
        return plane, F.normalize(camera_view[None].repeat(plane.shape[0], 1), dim=-1)
    if mode == 'persp':
        dirs = F.normalize(plane - camera_origin, dim=-1)
        return camera_origin.repeat(dirs.shape[0], 1), dirs
    raise ValueError('Invalid camera mode!')


def sdf_slice_colors(d):
    """The reference's colour map of a distance slice (offline_renderer.py:282-295), numpy [.., .] -> [.., ., 3]: orange inside,
    blue fading in outside over a dark yellow, light iso-lines every 0.04 of distance, a black zero crossing."""
    d = np.clip((d + 1.0) / 2.0, 0.0, 1.0)
    blue = np.clip((d - 0.5) * 2.0, 0.0, 1.0)
    vis = np.zeros([*d.shape, 3])
    vis[..., 2] = blue
    vis += (1.0 - blue)[..., None] * np.array([0.4, 0.3, 0.0])
    vis += 0.2
    vis[d - 0.5 < 0] = np.array([1.0, 0.38, 0.0])
    for i in range(50):
        vis[np.abs(d - 0.02 * i) < 0.0015] = 0.8
    vis[np.abs(d - 0.5) < 0.004] = 0.0
    return vis


def _is_field(fn):
    return hasattr(fn, "get_forward_function") and hasattr(fn, "grid")



class OfflineRenderer():
    def __init__(self,
        render_res   : Tuple[int, int] = (512, 512), # [w, h]
        render_batch : int  = -1, # -1 for no batching
        shading_mode : str  = 'rb',  # options: ['matcap', 'rb', 'normal']
        matcap_path  : str  = './data/matcap/Pearl.png',  # set if shading mode = matcap
        shadow       : bool = False,
        ao           : bool = False,
        perf         : bool = False,
        device       : torch.device = 'cuda'
    ):
        if shadow or ao:
            raise NotImplementedError("OfflineRenderer: the shadow and ambient-occlusion passes are not provided")
        self.render_res = render_res
        self.render_batch = render_batch
        self.shading_mode = shading_mode
        self.matcap_path = matcap_path
        self.shadow = shadow
        self.ao = ao
        self.perf = perf
        self.device = device
        self.width, self.height = self.render_res

    def render_lookat(self, pipeline, f=[0, 0, 1], t=[0, 0, 0], fov=30.0, camera_proj='persp', device='cuda', mm=None,
                      lod_idx=None, camera_clamp=[0, 5]):
        """RenderBuffer [height, width, .] of the pipeline seen from `f` towards `t`; mm: 3x3 model matrix the rays are taken
        through (row vectors times mm)."""
        ray_o, ray_d = _look_at(f, t, self.height, self.width, fov=fov, mode=camera_proj, device=device)
        if mm is not None:
            mm = mm.to(ray_o.device)
            ray_o, ray_d = torch.mm(ray_o, mm), torch.mm(ray_d, mm)
        rays = Rays(origins=ray_o, dirs=ray_d, dist_min=camera_clamp[0], dist_max=camera_clamp[1])
        return self.render(pipeline, rays, lod_idx=lod_idx).reshape(self.height, self.width, -1)

    def render(self, pipeline, rays, lod_idx=None):
        """Trace `rays` (in batches of render_batch when positive) and shade by shading_mode."""
        from wisp.tracers.packed_sdf_tracer import PackedSDFTracer
        if self.shading_mode not in ('matcap', 'rb', 'normal'):
            raise NotImplementedError
        start = time.time() if self.perf else None
        tracer = pipeline.tracer
        own = isinstance(tracer, PackedSDFTracer)
        had = own and "fused_normals" in vars(tracer)
        was = vars(tracer).get("fused_normals") if own else None
        if own:
            tracer.fused_normals = True                  # for these traces only: restored below
        try:
            with torch.no_grad():
                if self.render_batch > 0:
                    rb = RenderBuffer(xyz=None, hit=None, normal=None, shadow=None, ao=None, dirs=None)
                    for pack in rays.split(self.render_batch):
                        rb += tracer(pipeline.nef, rays=pack, lod_idx=lod_idx)
                else:
                    rb = tracer(pipeline.nef, rays=rays, lod_idx=lod_idx)
                if self.shading_mode == 'rb':
                    self._field_colours(pipeline.nef, rb, lod_idx)
        finally:
            if own:
                if had:
                    tracer.fused_normals = was
                else:
                    del tracer.fused_normals
        if self.perf:
            print("Time Elapsed:{:.4f}".format(time.time() - start))
        if self.shading_mode == 'matcap':
            rb = matcap_shader(rb, rays, self.matcap_path, mm=None)
        elif self.shading_mode == 'rb':
            assert rb.rgb is not None and "No rgb in buffer; change shading-mode"
        else:
            rb.rgb = (rb.normal + 1.0) / 2.0
        if rb.normal is not None:
            rb.normal[~rb.hit] = 1.0
        return rb

    @staticmethod
    def _field_colours(nef, rb, lod_idx):
        """'rb' on a field with a colour output: rgb at the hit points from the field, background left as traced"""
        from wisp.ops.sdf import is_textured, sdf_query
        if not is_textured(nef) or rb.xyz is None or rb.hit is None:
            return
        hit = rb.hit.reshape(-1).bool()
        rgb = torch.zeros(hit.shape[0], 3, device=rb.xyz.device) if rb.rgb is None else rb.rgb.reshape(-1, 3).clone()
        if bool(hit.any()):
            rgb[hit] = sdf_query(nef, rb.xyz.reshape(-1, 3)[hit], lod_idx)[:, :3].to(rgb.dtype)
        rb.rgb = rgb.reshape(*rb.xyz.shape[:-1], 3)

    def normal_slice(self, fn, dim=0, depth=0.0):
        """numpy [width, height, 3]: normal colours (n + 1) / 2 of the field on an axis-aligned plane"""
        pts = normalized_slice(self.width, self.height, dim=dim, depth=depth, device=self.device).reshape(-1, 3)
        if _is_field(fn):
            from wisp.ops.sdf import sdf_fd_gradient
            grad = sdf_fd_gradient(fn, pts, None)
        else:
            grad = finitediff_gradient(pts, fn).detach()
        normal = (F.normalize(grad) + 1.0) / 2.0
        return normal.reshape(self.width, self.height, 3).cpu().numpy()

    def sdf_slice(self, fn, dim=0, depth=0):
        """numpy [width, height, 3]: the colour-mapped distances of the field on an axis-aligned plane"""
        pts = normalized_slice(self.width, self.height, dim=dim, depth=depth, device=self.device)
        with torch.no_grad():
            if _is_field(fn):
                from wisp.ops.sdf import sdf_query
                d = sdf_query(fn, pts.reshape(-1, 3), None)[:, -1:]
            else:
                d = fn(pts.reshape(-1, 3))
        d = d.reshape(self.width, self.height, 1).squeeze().cpu().numpy()
        return sdf_slice_colors(d)

    def render_snapshot(self, pipeline, f=[0, 0, 1], t=[0, 0, 0], fov=30.0, aa=1, mm=None, lod_idx=None, camera_clamp=[0, 10]):
        """The image buffers of one view on the host, transposed to [width, height, .]; aa > 1 averages that many renders (the
        pixel grid is the same every time: the average equals a single render, as in the reference)."""
        if mm is None:
            mm = torch.eye(3)
        if aa > 1:
            rb = RenderBuffer.mean(*[self.render_lookat(pipeline, f=f, t=t, fov=fov, mm=mm, lod_idx=lod_idx, camera_clamp=camera_clamp)
                                     for _ in range(aa)])
        else:
            rb = self.render_lookat(pipeline, f=f, t=t, fov=fov, mm=mm, lod_idx=lod_idx, camera_clamp=camera_clamp)
        return rb.cpu().transpose()
