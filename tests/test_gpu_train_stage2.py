"""``python -m hesic_amd.train_stage2`` on a real MI355X: a synthetic folder (5 training and 2 validation pairs of 80 x 96 PNGs with sidecars,
built the way tests/test_gpu_pair_batch.py builds one), patch 64 x 64, batch 2, the frozen model on its synthetic weights."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from hesic_amd import codec, eval_folder, models, pair_cache, synthetic, train_stage2

pytestmark = pytest.mark.gpu
DEV = "cuda"
LAMBDA = 0.01


@pytest.fixture(autouse=True)
def _reset_dtype():
    import hesic_amd
    yield
    hesic_amd.set_compute_dtype(torch.bfloat16)
    hesic_amd.set_compute_dtype(torch.float32)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("stage2_pairs")
    for split, first, n in (("train", 300, 5), ("test", 400, 2)):
        for d in ("left", "right", "H"):
            (root / split / d).mkdir(parents=True)
        for i in range(n):
            x1, x2, H = synthetic.smooth_stereo_pair(first + i, 80, 96)
            q = codec.quantise(torch.from_numpy(np.stack([x1, x2])))
            Image.fromarray(q[0]).save(root / split / "left" / f"pair{i:02d}.png")
            Image.fromarray(q[1]).save(root / split / "right" / f"pair{i:02d}.png")
            np.save(root / split / "H" / f"pair{i:02d}.npy", H.astype(np.float64))
    return root


def _common(folder, out):
    return [str(folder), "--checkpoint", "synthetic", "--patch-size", "64", "64", "--batch-size", "2", "--test-batch-size", "2", "--seed", "1",
            "--save", "--out", str(out)]


@pytest.fixture(scope="module")
def full(folder, tmp_path_factory):
    """The uninterrupted two-epoch run: (records, output directory)."""
    out = tmp_path_factory.mktemp("stage2_full")
    logs = []
    hist = train_stage2.main(_common(folder, out) + ["-e", "2"], log=logs.append)
    assert len(hist) == 2 and len(logs) == 2
    return hist, out


def _golden_keys():
    with open(os.path.join(GOLDEN, "en_state_keys.txt")) as f:
        return [(line.split()[0], tuple(int(v) for v in line.split()[1:])) for line in f if line.strip()]


def test_two_epochs_write_both_checkpoints_in_the_references_format(full):
    hist, out = full
    assert [r["epoch"] for r in hist] == [0, 1] and all(r["steps"] == 3 and r["dropped_tail"] == 0 for r in hist)
    assert all(np.isfinite(r["train_loss"]) and np.isfinite(r["valid_loss"]) for r in hist)
    last = torch.load(out / "second_checkpoint.pth.tar", map_location="cpu")
    best = torch.load(out / "second_checkpoint_best_loss.pth.tar", map_location="cpu")
    assert set(last) == {"epoch", "state_dict", "loss", "optimizer", "aux_optimizer", "seed"} and last["epoch"] == 1 and last["seed"] == 1
    assert last["loss"] == hist[1]["valid_loss"] and best["loss"] == min(r["valid_loss"] for r in hist)
    assert {k: tuple(v.shape) for k, v in last["state_dict"].items()} == dict(_golden_keys()) and len(last["state_dict"]) == 80
    assert all(v.device.type == "cpu" and v.dtype == torch.float32 for v in last["state_dict"].values())
    assert last["aux_optimizer"]["state"] == {} and len(last["aux_optimizer"]["param_groups"]) == 1          # never stepped
    assert float(last["optimizer"]["state"][0]["step"]) == 6.0
    # the reference's Independent_EN().load_state_dict(...) contract, on the drop-in
    models.Independent_EN().load_state_dict(last["state_dict"], strict=True)
    en = eval_folder.load_enhancer(str(out / "second_checkpoint_best_loss.pth.tar"))
    assert not en.training and all(torch.equal(p.detach().cpu(), best["state_dict"][k]) for k, p in en.named_parameters())


def test_validation_record_is_the_criterion_and_the_frozen_models_rate(full, folder):
    hist, _ = full
    import hesic_amd
    for r in hist:
        v = r["valid"]
        assert v["batches"] == 1 and v["loss"] == pytest.approx(LAMBDA * 255 ** 2 * v["mse_loss"], rel=1e-12)
        assert v["psnr"] == (v["psnr1"] + v["psnr2"]) / 2 and "ms_ssim1" not in v
    # bpp_loss: the frozen model's own rate on the validation crops, whatever the enhancer has become
    assert hist[0]["valid"]["bpp_loss"] == pytest.approx(hist[1]["valid"]["bpp_loss"], rel=1e-9)
    net = codec.load_model(None, torch.float16)
    try:
        cache = pair_cache.DevicePairCache(str(folder), "test", mode="device")
        plan = pair_cache.epoch_plan(len(cache), cache.sizes, 2, 64, 64, 1, None, False, False)
        (indices, origins), = plan
        x1, x2, h, _ = cache.batch(indices, origins, 64, 64)
        with torch.no_grad():
            rd = models.rate_distortion(net(x1, x2, h), x1, x2)
        bpp = float(sum(v for k, v in rd.items() if k.startswith("bits_")).reshape(()) / rd["num_pixels"])
    finally:
        hesic_amd.set_compute_dtype(torch.float32)
    print(f"train_stage2 valid bpp_loss: record {hist[1]['valid']['bpp_loss']!r} by hand {bpp!r}")
    assert hist[1]["valid"]["bpp_loss"] == pytest.approx(bpp, rel=1e-9)


def test_graphed_run_drops_the_ragged_tail_and_counts_it(folder, tmp_path):
    hist = train_stage2.main(_common(folder, tmp_path)[:-3] + ["-e", "2", "--graphed"], log=lambda s: None)
    assert [r["steps"] for r in hist] == [2, 2] and [r["dropped_tail"] for r in hist] == [1, 1]
    assert all(np.isfinite(r["train_loss"]) and np.isfinite(r["valid_loss"]) for r in hist)
    assert not (tmp_path / "second_checkpoint.pth.tar").exists()                  # --save is off


def test_resumed_run_equals_the_uninterrupted_run_bit_for_bit(full, folder, tmp_path):
    hist, out = full
    first = train_stage2.main(_common(folder, tmp_path) + ["-e", "1"], log=lambda s: None)
    assert first[0]["valid"] == hist[0]["valid"] and first[0]["train"] == hist[0]["train"]
    more = train_stage2.main(_common(folder, tmp_path)[:-5] + ["--save", "--out", str(tmp_path), "-e", "2", "--resume",
                                                               str(tmp_path / "second_checkpoint.pth.tar")], log=lambda s: None)
    assert [r["epoch"] for r in more] == [1]
    a = torch.load(out / "second_checkpoint.pth.tar", map_location="cpu")
    b = torch.load(tmp_path / "second_checkpoint.pth.tar", map_location="cpu")
    assert b["epoch"] == 1 and b["seed"] == 1
    for k, v in a["state_dict"].items():
        assert torch.equal(v.view(torch.int32), b["state_dict"][k].view(torch.int32)), k
    for i, st in a["optimizer"]["state"].items():
        for name in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(st[name].cpu().view(torch.int32), b["optimizer"]["state"][i][name].cpu().view(torch.int32)), (i, name)
    assert more[0]["valid"] == hist[1]["valid"] and more[0]["train"] == hist[1]["train"]
