"""Host mirror of the reference's offline buffer assembly (data_gen/*.py) on libnlt_hip.so.
Same function names and argument meaning as the reference; tensors are torch CUDA tensors.
The Cycles renders stay out of scope: a capture made in Blender hands its OUTPUTS (per-pixel hit position / normal / face
index, occlusion flags, the unwrap table) to this package.  Without Blender, mesh.py casts the rays itself, shade.py / rig.py /
capture_main.py render a capture of their own from a mesh (not Cycles) and unwrap.py unwraps the mesh (smart projection restated,
not Blender's result)."""
from . import util, render, get_neighbors, postproc      # noqa: F401
