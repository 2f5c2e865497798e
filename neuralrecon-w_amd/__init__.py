"""neuralrecon-w_amd: MI355X (gfx950) native volume-rendering hot path of NeuralRecon-W.

Drop-in for the reference's `models.neuconw.NeuconW`, `models.nerf.NeRF` and
`rendering.renderer.NeuconWRenderer`.  All per-sample compute is in
libneuconw_hip.so (hand-written HIP, C ABI in include/neuconw_hip.h).

The names below are bound on first use (PEP 562), not at import time, so that the file readers (`colmap`, `ply`) import without
torch.  `import neuralrecon_w_amd` alone therefore loads nothing: a missing module or library shows at the first name used.
"""
import importlib

_SUBMODULES = ("lib", "mesh", "evalmesh", "reproj", "views", "appfit", "align")
_HOME = {"PREC_BF16": "lib", "PREC_F16": "lib", "PREC_F32": "lib", "NeuconwHipError": "lib", "NeRF": "nerf", "NeuconW": "neuconw",
         "RenderingNetwork": "neuconw", "SDFNetwork": "neuconw", "SingleVarianceNetwork": "neuconw", "NeuconWRenderer": "renderer",
         "NeuconWLoss": "losses", "FlatAdam": "trainer", "FlatParams": "trainer", "TrainStep": "trainer", "Camera": "views",
         "render_view": "views", "scene_view": "views", "write_panel": "views"}


def __getattr__(name):
    if name in _SUBMODULES:
        return importlib.import_module("." + name, __name__)
    if name in _HOME:
        value = globals()[name] = getattr(importlib.import_module("." + _HOME[name], __name__), name)
        return value
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
