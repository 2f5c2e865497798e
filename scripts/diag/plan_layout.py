"""CPU: one hash per pack plan of the three networks (SDF widths 64 / 256 / 512 x f32 / bf16 / f16) over the arena layout
(_mats, _biases, _dense, _dense_b) and the pack / unpack descriptors with every tensor replaced by its parameter's name.
A change to the host code that builds the plans must leave all 27 lines as they are."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from neuralrecon_w_amd import lib as L  # noqa: E402
from tests._build import build_system  # noqa: E402

for W in (64, 256, 512):
    kw = {} if W == 64 else dict(color_hidden=256, head=128, nerf_w=256)
    _, neuconw, nerf, _ = build_system(W=W, device="cpu", **kw)
    for pname, prec in (("f32", L.PREC_F32), ("bf16", L.PREC_BF16), ("f16", L.PREC_F16)):
        for tag, mod in (("sdf", neuconw.sdf_net), ("color", neuconw.color_net), ("nerf", nerf)):
            plan = mod.plan(prec)
            names = {id(p): k for k, p in mod.named_parameters()}
            descs = [sorted((k, names[id(v)] if torch_like else v) for k, v in d.items()
                            for torch_like in [hasattr(v, "data_ptr")])
                     for d in plan._pack + plan._unpack]
            text = repr((plan._mats, plan._biases, plan._dense, plan._dense_b, len(plan._pack), descs))
            print("W=%d %-4s %-5s %s" % (W, pname, tag, hashlib.sha256(text.encode()).hexdigest()[:16]))
