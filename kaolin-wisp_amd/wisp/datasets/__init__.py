from .batch import Batch, MultiviewBatch, SDFBatch
from .transforms import SampleRays
from .multiview_tensor_dataset import MultiviewTensorDataset
from .sdf_tensor_dataset import SDFTensorDataset
from .image_dataset import ImageDataset
from .base_datasets import SDFDataset, MultiviewDataset
from .formats import MeshSampledSDFDataset, OctreeSampledSDFDataset, NeRFSyntheticDataset
from .utils import load_multiview_dataset
