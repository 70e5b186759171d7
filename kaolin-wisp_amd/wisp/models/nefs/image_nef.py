"""ImageNeuralField (app/image): pixel coordinates -> hash-grid features (+) 3-octave embedding -> MLP -> sigmoid RGB.
Mirrors wisp/models/nefs/image_nef.py:35-97; `rgb()` hands back the tensor itself because ImageTrainer consumes it that
way (wisp/trainers/image_trainer.py:66)."""
import torch

from wisp.models.grids import BLASGrid
from wisp.models.nefs import _grid_mlp
from wisp.models.nefs.base_nef import BaseNeuralField

_OCTAVES = 3


class ImageNeuralField(BaseNeuralField):
    def __init__(self, grid: BLASGrid, activation_type: str = 'relu', layer_type: str = 'none', hidden_dim: int = 128,
                 num_layers: int = 1):
        super().__init__()
        self.grid = grid
        self.activation_type, self.layer_type = activation_type, layer_type
        self.hidden_dim, self.num_layers = hidden_dim, num_layers
        n_lods = len(grid.resolutions)
        self.feature_dim = grid.feature_dim * (n_lods if grid.multiscale_type == 'cat' else 1)
        self.embedder, self.embed_dim = _grid_mlp.make_position_embedder('positional', _OCTAVES, True, coord_dim=2)
        self.input_dim = self.feature_dim + self.embed_dim
        self.decoder = _grid_mlp.make_decoder(self.input_dim, 3, activation_type, layer_type, num_layers, hidden_dim)

    def register_forward_functions(self):
        self._register_forward_function(self.rgb, ["rgb"])

    def rgb(self, coords, lod=None):
        """coords [batch, 2] in [-1, 1] -> colours [batch, 3] in (0, 1)."""
        lod = len(self.grid.resolutions) - 1 if lod is None else lod
        return torch.sigmoid(_grid_mlp.decode(self.grid, self.decoder, self.embedder, coords, lod, embed_first=False))

    def render_image(self, h, w, first=0, count=None, out='f32', gts_u8=None, lod=None, chunk=1000000):
        """The module-level render_image over this field."""
        return render_image(self, h, w, first, count, out, gts_u8, lod, chunk)


# ---------------------------------------------------------------------------------------------- whole-image render
def fused_render_shape(nef):
    """What wisp_image_field_render evaluates, or None when this field is not its shape: a 'cat' HashGrid without a BLAS, two
    fp32 features per entry, at most 16 levels; a BasicDecoder of one hidden relu Linear layer of at most 128 units with
    biases and 3 outputs; this class's own 3-octave embedder - all on the GPU.  WISP_IMAGE_RENDER_FUSED=0 declines."""
    import os
    from wisp.models.decoders import BasicDecoder
    from wisp.models.embedders import PositionalEmbedder
    from wisp.models.grids import HashGrid
    grid, dec, emb = getattr(nef, 'grid', None), getattr(nef, 'decoder', None), getattr(nef, 'embedder', None)
    if os.environ.get("WISP_IMAGE_RENDER_FUSED", "1") == "0" or type(grid) is not HashGrid or grid.blas is not None or not isinstance(nef, ImageNeuralField):
        return None
    table = grid.codebook.feats
    if not (grid.multiscale_type == 'cat' and grid.feature_dim == 2 and 1 <= grid.num_lods <= 16 and table.is_cuda
            and table.dtype == torch.float32 and table.is_contiguous()):
        return None
    if not (type(emb) is PositionalEmbedder and emb.num_freq == _OCTAVES and emb.include_input and emb.log_sampling
            and emb.max_freq_log2 == _OCTAVES - 1):
        return None
    layers, lout = getattr(dec, 'layers', None), getattr(dec, 'lout', None)
    if not (type(dec) is BasicDecoder and layers is not None and len(layers) == 1 and not dec.skip
            and type(layers[0]) is torch.nn.Linear and type(lout) is torch.nn.Linear and layers[0].bias is not None
            and lout.bias is not None and lout.out_features == 3 and layers[0].out_features <= 128
            and layers[0].in_features == 2 * grid.num_lods + 14 and layers[0].weight.dtype == torch.float32
            and layers[0].weight.is_cuda and dec.activation in (torch.relu, torch.nn.functional.relu)):
        return None
    return grid, layers[0], lout

def render_image(nef, h, w, first=0, count=None, out='f32', gts_u8=None, lod=None, chunk=1000000):
    """Colours of pixels [first, first + count) of the h x w image the field `nef` (anything with ImageNeuralField.rgb) was fitted to (row-major; count None = to the
    end), coordinates as normalized_grid(h, w, use_aspect=False) gives them: [count, 3], fp32 for out='f32', or u8
    `(rgb * 255).byte()` for out='u8'.  With `gts_u8` (the u8 [h, w, 3] ground truth on the field's device) the result is
    (image, sum of squared errors against gts / 255 as a float64 scalar tensor).
    One launch of the fused kernel (csrc/image_field.hip) when the field is its shape, `rgb()` over `chunk` coordinates at a
    time otherwise - same outputs."""
    if out not in ('f32', 'u8'):
        raise ValueError(f"out must be 'f32' or 'u8', got {out!r}")
    count = h * w - first if count is None else count
    if first < 0 or count < 0 or first + count > h * w:
        raise ValueError(f"pixels [{first}, {first + count}) leave the {h} x {w} image")
    if lod is not None and not 0 <= lod <= len(nef.grid.resolutions):
        raise ValueError(f"lod must be in 0 .. {len(nef.grid.resolutions)} (the number of levels rgb() blends), got {lod}")
    fused = fused_render_shape(nef)
    if fused is not None:
        import wisp._C as _C
        grid, l1, lout = fused
        packed, hp = _C.image_field_pack_weights(l1.weight, l1.bias, lout.weight, lout.bias, grid.num_lods)
        f32, u8, part = _C.image_field_render(h, w, first, count, grid.codebook.feats.detach(), grid.codebook.begin_idxes,
                                              grid.codebook.resolutions.reshape(-1).tolist(), grid.codebook_bitwidth,
                                              grid.num_lods - 1 if lod is None else lod, packed, hp, gts_u8=gts_u8,
                                              want_f32=out == 'f32', want_u8=out == 'u8', want_err=gts_u8 is not None)
        img = f32 if out == 'f32' else u8
        return img if gts_u8 is None else (img, part.sum())
    device = next(nef.parameters()).device
    pieces, err = [], torch.zeros((), dtype=torch.float64, device=device)
    gts_flat = None if gts_u8 is None else gts_u8.reshape(-1, 3)
    with torch.no_grad():
        for a in range(first, first + count, chunk):
            b = min(a + chunk, first + count)
            xy = _pixel_coords(h, w, a, b, device)
            rgb = (nef.rgb(xy) if lod is None else nef.rgb(xy, lod)).detach()
            if gts_flat is not None:
                d = rgb - gts_flat[a:b].to(device) / 255.0
                err += (d * d).double().sum()
            pieces.append(rgb if out == 'f32' else (rgb * 255).byte())
    img = torch.cat(pieces) if pieces else torch.zeros(0, 3, dtype=torch.float32 if out == 'f32' else torch.uint8, device=device)
    return img if gts_u8 is None else (img, err)


def _pixel_coords(h, w, a, b, device):
    """normalized_grid(h, w, use_aspect=False).reshape(-1, 2)[a:b] without the grid: the sampling kernel's own coordinates on the
    GPU, torch's linspace on the host (the two agree bit for bit, include/wisp_hip.h)."""
    idx = torch.arange(a, b, dtype=torch.int64, device=device)
    if torch.device(device).type == 'cuda':
        import wisp._C as _C
        return _C.image_sample(None, idx, want=("coords",), size=(h, w))["coords"]
    xs = torch.linspace(-1, 1, steps=w)
    ys = torch.linspace(1, -1, steps=h)
    return torch.stack([xs[idx % w], ys[idx // w]], dim=-1)
