"""What a snowpack knows of the terrain around it (counterpart of smrt/core/terrain.py: TerrainInfo).  The nadir_sar_altimetry
solver reads `snowpack.terrain_info`: the distribution of the surface elevation and its standard deviation `sigma_surface` (m)."""
from dataclasses import dataclass
from typing import Optional

import numpy as np


@dataclass
class TerrainInfo:
    distribution: str = "normal"
    sigma_surface: float = 0.0
    slope_angle: float = 0.0
    slope_direction: float = 0.0
    dem: Optional[np.ndarray] = None
