"""Generate tests/golden/lidar_sim_fixture.pt: beam tables and rays of the REFERENCE's own simulated LiDAR
(``app/resources/observers/lidars.py``, loaded unchanged from where it lies).

  * ``SurroundLidarGenerator`` / ``SolidStateLidarGenerator`` are driven on the CPU (``set_device``, ``set_dtype``) for pandar64
    (irregular table, 64 x 1800), vlp16, ruby128 (128 x 3600), bpearl (the axis variant) and rs_m1; what is stored of them is
    DATA: ``thetas``, ``phis`` as the f32 tensors the generator feeds its meshgrid, ``near``, ``far``.  Of rs_m1's 115 010
    (theta, phi) pairs every 25th is kept;
  * ``Lidar.get_all_rays`` (lidars.py:208-249) is called unbound on a stand-in node that carries the generator and a
    ``world_transform`` -- for two poses: a rotation + translation, and the same with a non-unit scale.  Stored are the rays at 4096
    seeded ray indices per sensor (for rs_m1 among the kept pairs), not whole sweeps; ``rays_o`` is one row, after the generator
    checked that the reference's tile repeats it for every ray.
``RisleyPrismLidarGenerator`` is never constructed (its constructor downloads a zip when its data directory is empty).

Runs in the authoring container only.   python tests/golden/make_lidar_sim_fixture.py
"""
import importlib.util
import math
import sys
import types
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
REF = Path("/root/reference")
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

SENSORS = [("Surround", "pandar64"), ("Surround", "vlp16"), ("Surround", "ruby128"), ("Surround", "bpearl"),
           ("Solid_state", "rs_m1")]
N_IDX = 4096
KEEP_EVERY = 25


def _load_lidars():
    """the reference's lidars.py with the shim's nr3d_lib and a bare SceneNode"""
    import nr3d_lib.fmt  # noqa: F401
    import nr3d_lib.utils  # noqa: F401
    for name in ("app", "app.resources", "app.resources.observers"):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    nodes = types.ModuleType("app.resources.nodes")
    nodes.SceneNode = type("SceneNode", (), {})
    sys.modules["app.resources.nodes"] = nodes
    spec = importlib.util.spec_from_file_location("app.resources.observers.lidars", str(REF / "app/resources/observers/lidars.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


class _Pose:
    def __init__(self, m):
        self.m = m

    def mat_4x4(self):
        return self.m


def _generator(mod, model, name):
    """the reference's generator on the CPU.  The constructors select a default unit before a device can be set (the solid-state
    one builds tensors on its default device there), so the object is made first and initialised by the base class."""
    cls = {"Surround": mod.SurroundLidarGenerator, "Solid_state": mod.SolidStateLidarGenerator}[model]
    g = cls.__new__(cls)
    mod.AbstractLidarGenerator.__init__(g, model)
    g.set_device(torch.device("cpu"))
    g.set_dtype(torch.float)
    g.select_lidar_by_name(name)
    return g


def _node(mod, gen, pose):
    n = types.SimpleNamespace(i_prefix=(), device=torch.device("cpu"), dtype=torch.float, lidar_generator=gen,
                              world_transform=_Pose(pose), thetas=gen.thetas, phis=gen.phis)
    c = torch.eye(4)
    c[:3, :3] = torch.tensor([[0.0, 1, 0], [0, 0, -1], [1, 0, 0]])      # the node's carla_to_opencv (lidars.py:188-192)
    n.carla_to_opencv = c
    return n


def poses():
    ax = torch.tensor([0.3, -0.5, 0.81], dtype=torch.float64)
    ax = ax / ax.norm()
    K = torch.tensor([[0.0, -ax[2], ax[1]], [ax[2], 0.0, -ax[0]], [-ax[1], ax[0], 0.0]], dtype=torch.float64)
    a = 0.83
    R = torch.eye(3, dtype=torch.float64) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)
    out = {}
    for tag, s in (("rigid", 1.0), ("scaled", 1.7)):
        m = torch.eye(4, dtype=torch.float64)
        m[:3, :3] = R * s
        m[:3, 3] = torch.tensor([12.5, -3.25, 1.875], dtype=torch.float64)
        out[tag] = m.to(torch.float32)
    return out


def main():
    mod = _load_lidars()
    assert "RisleyPrismLidarGenerator" in dir(mod)          # present, and never constructed
    P = poses()
    sensors, rays = [], {}
    for k, (model, name) in enumerate(SENSORS):
        gen = _generator(mod, model, name)
        Ts, Ps = gen.get_Ts_Ps()
        grid = model == "Surround"
        if grid:
            thetas, phis = Ts[0].clone(), Ps[:, 0].clone()          # meshgrid 'xy': Ts[i, j] = thetas[j], Ps[i, j] = phis[i]
            assert torch.equal(Ts, thetas[None, :].expand_as(Ts)) and torch.equal(Ps, phis[:, None].expand_as(Ps))
            n_total = Ts.numel()
        else:
            n_total = Ts.numel()
            kept = torch.arange(0, n_total, KEEP_EVERY)
            thetas, phis = Ts[kept].clone(), Ps[kept].clone()
        g = torch.Generator().manual_seed(1000 + k)
        if grid:
            idx = torch.randperm(n_total, generator=g)[:N_IDX].sort().values
            ref_idx = idx
        else:
            idx = torch.randperm(kept.numel(), generator=g)[:N_IDX].sort().values          # indices among the kept pairs
            ref_idx = kept[idx]
        sensors.append(dict(lidar_model=model, lidar_name=name, mode="grid" if grid else "paired",
                            axis=1 if name == "bpearl" else 0, near=float(gen.near), far=float(gen.far),
                            thetas=thetas.to(torch.float32).contiguous(), phis=phis.to(torch.float32).contiguous()))
        for tag, pose in P.items():
            o, d, tp = mod.Lidar.get_all_rays(_node(mod, gen, pose), return_theta_phi=True)
            assert o.shape == d.shape == (n_total, 3) and bool((o == o[0]).all())
            tp = tp.reshape(-1, 2)[ref_idx]
            assert torch.equal(tp[:, 0], (thetas[idx % thetas.numel()] if grid else thetas[idx]))
            rays[(name, tag)] = dict(rays_o=o[0].clone(), rays_d=d[ref_idx].clone().contiguous())
        sensors[-1]["idx"] = idx.to(torch.int32)
    out = dict(sensors=sensors, poses={k: v.clone() for k, v in P.items()},
               rays={f"{n}/{t}": v for (n, t), v in rays.items()}, keep_every=KEEP_EVERY)
    path = HERE / "lidar_sim_fixture.pt"
    torch.save(out, path)
    print("wrote", path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
