from .conversions import *
from .processing import *
