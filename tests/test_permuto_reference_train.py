"""The reference's OWN trainer (``code_single/tools/train.py``, source unchanged, run by tools/run_reference_train.py) on its
permutohedral recipe, code_single/configs/object_centric/permuto_neus.bmvs.230814.yaml: ``PermutoNeuSObj`` main model +
``PermutoNeRFDistant`` background, both lattices annealed (``anneal_cfg{type: hardmask}``), image embeddings.  Sizes are shrunk
through the trainer's own ``--a.b.c=value`` overrides, as tests/test_reference_train.py does for the LoTD object config.

Authoring container only (needs the reference's sources; emulator backend)."""
import pickle
from pathlib import Path

import torch

import ref_glue
import test_reference_train as trt

CFG = trt.REF / "code_single/configs/object_centric/permuto_neus.bmvs.230814.yaml"
needs_reference = ref_glue.needs_reference(ref_glue.readable(CFG), reason="executes the reference's own sources, which only the authoring machine has (emulator backend)")

M, D = trt.M, trt.D
SMALL = [
    "--dataset_cfg.target=neuralsim_amd.dataio.SyntheticObjectDataset", "--dataset_cfg.param.n_frames=6",
    "--dataset_cfg.param.image_hw=32", "--num_rays=96", "--num_coarse=8", "--num_fine=[4,4]",
    "--upsample_inv_s_factors=[1,4]", "--step_size=0.05", "--bgsample=8",
    f"--{M}.surface_cfg.encoding_cfg.permuto_auto_compute_cfg.n_levels=8",
    f"--{M}.surface_cfg.encoding_cfg.permuto_auto_compute_cfg.log2_hashmap_size=12",
    f"--{M}.surface_cfg.encoding_cfg.permuto_auto_compute_cfg.coarsest_res=2.0",
    f"--{M}.surface_cfg.encoding_cfg.permuto_auto_compute_cfg.finest_res=32.0", f"--{M}.accel_cfg.resolution=[16,16,16]",
    f"--{M}.accel_cfg.init_cfg.num_pts=4096", f"--{M}.accel_cfg.init_cfg.num_steps=2",
    f"--{M}.accel_cfg.update_from_net_cfg.num_pts=4096", f"--{M}.accel_cfg.update_from_net_cfg.num_steps=1",
    f"--{M}.accel_cfg.n_steps_warmup=2", f"--{M}.accel_cfg.n_steps_between_update=2",
    f"--{M}.ray_query_cfg.query_param.march_cfg.max_steps=128",
    "--assetbank_cfg.Main.asset_params.initialize_cfg.num_iters=10", "--assetbank_cfg.Main.asset_params.initialize_cfg.lr=5.0e-3",
    f"--{D}.encoding_cfg.permuto_auto_compute_cfg.n_levels=6", f"--{D}.encoding_cfg.permuto_auto_compute_cfg.log2_hashmap_size=10",
    f"--{D}.encoding_cfg.permuto_auto_compute_cfg.coarsest_res=2.0", f"--{D}.encoding_cfg.permuto_auto_compute_cfg.finest_res=24.0",
    "--stop_it=5", "--bg_stop_it=5",                       # both annealing schedules end inside the run
    "--training.i_save=-1", "--training.i_backup=-1", "--training.uniform_sample.Main=64",
]


@needs_reference
def test_reference_trainer_runs_the_permuto_recipe(tmp_path, monkeypatch):
    monkeypatch.setattr(trt, "CFG", CFG)
    monkeypatch.setattr(trt, "SMALL", SMALL)
    exp = tmp_path / "exp"
    r = trt._run(exp, ["--num_iters=6", "--training.i_val=-1", "--training.i_log=1"])
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0 and "Everything done." in r.stdout, tail
    ck = sorted((exp / "ckpts").glob("final_*.pt"))
    assert len(ck) == 1 and ck[0].name == "final_00000006.pt"
    bank = torch.load(str(ck[0]), map_location="cpu", weights_only=False)["asset_bank"]
    assert any(k.startswith("PermutoNeuSObj#Main") for k in bank), list(bank)
    assert any(k.startswith("ImageEmbeddings#") for k in bank), list(bank)
    dist = next(v for k, v in bank.items() if k.startswith("PermutoNeRFDistant#Distant"))
    table = next(v for k, v in dist.items() if k.endswith("flattened_params"))
    # the table of ``Distant`` changed: its initial value is the constructor's (seed 7, ``param_init_cfg.bound`` 1e-4)
    init = ((torch.rand(table.numel(), generator=torch.Generator().manual_seed(7)) * 2 - 1) * 1e-4).half().float()
    assert table.shape == (6 * 2 ** 10 * 2,) and not torch.equal(table.float(), init)
    stats = pickle.loads((exp / "stats.p").read_bytes())
    for name, first, last in (("PermutoNeuSObj", 3, 8), ("PermutoNeRFDistant", 1, 6)):   # start_level 2 / -1 -> all levels
        n = [v for _, v in stats[f"anneal/{name}.n_active_levels"]]
        assert n[0] == first and n[-1] == last and n == sorted(n), (name, n)
    loss = [v for _, v in stats[next(k for k in stats if k.endswith("loss_rgb"))]]
    assert len(loss) >= 6 and all(l == l and l < 10 for l in loss), loss
