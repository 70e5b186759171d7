from .base_nef import *
from .nerf import *
from .neural_sdf import *
from .image_nef import *
from .neural_sdf_tex import *
from .spc_field import *
