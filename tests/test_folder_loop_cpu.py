"""``hesic_amd.folder_loop`` -- what ``train_folder`` and ``train_stage2`` share -- and ``train``'s one validation of the step controls, on the
host: the cache and the trainer are plain torch CPU stand-ins (``pair_cache.epoch_plan`` is host code).  The expected parser values and record
keys are written out: they are what the two commands had when each carried its own copy."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from hesic_amd import folder_loop, homography_train, pair_cache, train, train_folder, train_stage2

COMMANDS = [train_folder, train_stage2]
IDS = ["train_folder", "train_stage2"]
SIZES = [(80, 96)] * 5


class _Cache:
    """``device``, ``batch`` and what ``run_epochs`` reads of a ``DevicePairCache``."""
    device = torch.device("cpu")
    decode_seconds = 0.25

    def __init__(self, sizes=SIZES):
        self.sizes, self.calls = list(sizes), []

    def __len__(self):
        return len(self.sizes)

    def batch(self, indices, origins, ph, pw, out=None, flags=None):
        self.calls.append((list(indices), list(origins), flags))
        if out is not None:
            return (*out, None)
        x = torch.zeros(len(indices), 3, ph, pw)
        return x, x.clone(), torch.eye(3).repeat(len(indices), 1, 1), None


class _Trainer:
    """``step`` number ``s`` (from 0) returns ``keys[j]`` = ``values[s][j]`` as 0-dim fp32 tensors."""

    def __init__(self, keys, values, static=None):
        self.keys, self.values, self.s = keys, values, 0
        if static is not None:
            self.static_inputs = lambda: static

    def step(self, x1, x2, h):
        row, self.s = self.values[self.s], self.s + 1
        return {k: torch.tensor(v, dtype=torch.float32) for k, v in zip(self.keys, row)}


def _values(steps, n):
    g = np.random.Generator(np.random.PCG64([3, steps, n]))
    return g.uniform(0.1, 4.0, size=(steps, n)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------- the epoch pass
@pytest.mark.parametrize("mod", COMMANDS, ids=IDS)
def test_epoch_pass_means_steps_and_key_order(mod):
    plan = pair_cache.epoch_plan(5, SIZES, 2, 64, 64, 0, 0, True, False)
    assert len(plan) == 3
    vals = _values(3, len(mod.TRAIN_KEYS))
    got, steps, secs = mod.train_epoch(_Trainer(mod.TRAIN_KEYS, vals), _Cache(), plan, 64, 64)
    assert steps == len(plan) == 3 and secs >= 0
    assert list(got) == list(mod.TRAIN_KEYS)
    v = vals.astype(np.float64)
    assert list(got.values()) == ((v[0] + v[1] + v[2]) / 3).tolist()                 # the fp64 mean of the fp32 values, added in step order


@pytest.mark.parametrize("mod", COMMANDS, ids=IDS)
def test_epoch_pass_takes_a_plan_made_by_hand_and_passes_the_flags_of_a_planned_one(mod):
    by_hand = pair_cache.Plan([([0, 1], [(0, 0), (3, 5)]), ([2], [(1, 1)])])             # no ``flags``, no ``rng``
    cache = _Cache()
    got, steps, _ = mod.train_epoch(_Trainer(mod.TRAIN_KEYS, _values(2, len(mod.TRAIN_KEYS))), cache, by_hand, 64, 64)
    assert steps == 2 and [c[2] for c in cache.calls] == [None, None]
    planned = pair_cache.epoch_plan(5, SIZES, 2, 64, 64, 0, 0, True, False, augment=("hflip", "swap"))
    cache = _Cache()
    mod.train_epoch(_Trainer(mod.TRAIN_KEYS, _values(3, len(mod.TRAIN_KEYS))), cache, planned, 64, 64)
    assert [c[2] for c in cache.calls] == planned.flags and [c[0] for c in cache.calls] == [b[0] for b in planned]


@pytest.mark.parametrize("mod,name", list(zip(COMMANDS, IDS)), ids=IDS)
def test_epoch_pass_refuses_a_batch_of_another_size_than_the_captured_step(mod, name):
    plan = pair_cache.epoch_plan(5, SIZES, 2, 64, 64, 0, 0, True, False)
    static = (torch.zeros(4, 3, 64, 64), torch.zeros(4, 3, 64, 64), torch.zeros(4, 3, 3))
    with pytest.raises(RuntimeError) as e:
        mod.train_epoch(_Trainer(mod.TRAIN_KEYS, _values(3, len(mod.TRAIN_KEYS)), static), _Cache(), plan, 64, 64)
    assert str(e.value) == f"{name}: a batch of 2 for a step captured with 4"


def test_epoch_pass_writes_into_the_static_inputs():
    plan = pair_cache.epoch_plan(4, SIZES[:4], 2, 64, 64, 0, 0, True, True)
    static = (torch.zeros(2, 3, 64, 64), torch.zeros(2, 3, 64, 64), torch.zeros(2, 3, 3))
    seen = []

    class T(_Trainer):
        def step(self, x1, x2, h):
            seen.append(all(a is b for a, b in zip((x1, x2, h), static)))
            return super().step(x1, x2, h)

    folder_loop.train_epoch(T(("loss",), _values(2, 1), static), _Cache(), plan, 64, 64, ("loss",), "x")
    assert seen == [True, True]


# ------------------------------------------------------------------------------------------------------- the validation accumulator
def test_valid_epoch_means_both_psnr_forms_and_batches():
    keys = ("loss", "mse_loss", "psnr1", "psnr2")
    plan = pair_cache.epoch_plan(5, SIZES, 2, 64, 64, 0, None, False, False)
    vals, grads = torch.from_numpy(_values(3, 4)).double(), []

    def batch_values(x1, x2, h):
        grads.append(torch.is_grad_enabled())
        return vals[len(grads) - 1]

    rec = folder_loop.valid_epoch(_Cache(), plan, 64, 64, keys, batch_values)
    assert list(rec) == [*keys, "psnr", "psnr_of_mse", "batches"] and grads == [False] * 3
    want = (vals.sum(0) / 3).tolist()
    assert [rec[k] for k in keys] == want
    assert rec["psnr"] == (want[2] + want[3]) / 2
    assert rec["psnr_of_mse"] == folder_loop.mse2psnr(want[1] / 2) == 10 * math.log10(1 / (want[1] / 2))
    assert rec["batches"] == 3


def test_valid_epoch_of_an_empty_plan():
    rec = folder_loop.valid_epoch(_Cache(), pair_cache.Plan(), 64, 64, ("loss", "mse_loss", "psnr1", "psnr2"), lambda *a: 1 / 0)
    assert rec["batches"] == 0 and math.isnan(rec["psnr_of_mse"]) and rec["loss"] == 0.0


def test_each_commands_validation_record_and_its_late_lookup_of_valid_batch_values(monkeypatch):
    plan = pair_cache.epoch_plan(2, SIZES[:2], 2, 64, 64, 0, None, False, False)
    monkeypatch.setattr(train_folder, "valid_batch_values", lambda model, x1, x2, h, lmbda, distortion: torch.arange(1, 7).double())
    rec = train_folder.test_epoch(torch.nn.Identity(), _Cache(), plan, 64, 64, 0.01)
    assert list(rec) == ["loss", "mse_loss", "bpp_loss", "aux_loss", "psnr1", "psnr2", "psnr", "psnr_of_mse", "batches"]
    assert rec["loss"] == 1.0 and rec["psnr"] == 5.5
    monkeypatch.setattr(train_stage2, "valid_batch_values",
                        lambda model, en, x1, x2, h, lmbda, with_ms_ssim: torch.arange(1, 8 if with_ms_ssim else 6).double())
    rec = train_stage2.test_epoch(torch.nn.Identity(), torch.nn.Identity(), _Cache(), plan, 64, 64, 0.01)
    assert list(rec) == ["loss", "mse_loss", "bpp_loss", "psnr1", "psnr2", "psnr", "psnr_of_mse", "batches"]
    big = pair_cache.epoch_plan(1, [(192, 192)], 1, 192, 192, 0, None, False, False)
    rec = train_stage2.test_epoch(torch.nn.Identity(), torch.nn.Identity(), _Cache([(192, 192)]), big, 192, 192, 0.01)
    assert list(rec) == ["loss", "mse_loss", "bpp_loss", "psnr1", "psnr2", "ms_ssim1", "ms_ssim2", "psnr", "psnr_of_mse", "batches"]


# ------------------------------------------------------------------------------------------------------------- the resume position
def _ckpt(path, epoch, loss):
    path.parent.mkdir(parents=True, exist_ok=True)
    torch.save({"epoch": epoch, "loss": loss}, path)
    return torch.load(path)


def test_resume_position_without_a_resume(tmp_path):
    assert folder_loop.resume_position(None, "none", tmp_path / "c_best_loss.pth.tar", True) == (0, float("inf"))
    assert list(tmp_path.iterdir()) == []


@pytest.mark.parametrize("copy_best", [True, False], ids=["saving", "not-saving"])
def test_resume_position_reads_the_sibling_best_file_and_copies_it_only_when_asked(tmp_path, copy_best):
    old, new = tmp_path / "old", tmp_path / "new"
    new.mkdir()
    resume = _ckpt(old / "c.pth.tar", 4, 2.5)
    best = new / "c_best_loss.pth.tar"
    assert folder_loop.resume_position(resume, old / "c.pth.tar", best, copy_best) == (5, 2.5)          # no sibling
    _ckpt(old / "c_best_loss.pth.tar", 2, 1.5)
    assert folder_loop.resume_position(resume, str(old / "c.pth.tar"), best, copy_best) == (5, 1.5)     # the sibling's lower loss
    assert best.is_file() == copy_best
    if copy_best:
        assert torch.load(best) == {"epoch": 2, "loss": 1.5}
    _ckpt(old / "c_best_loss.pth.tar", 3, 3.5)                                                          # a higher one does not count
    assert folder_loop.resume_position(resume, old / "c.pth.tar", best, copy_best) == (5, 2.5)
    if copy_best:
        assert torch.load(best) == {"epoch": 2, "loss": 1.5}                                            # an existing target is left alone


def test_resume_position_does_not_copy_a_file_onto_itself(tmp_path):
    resume = _ckpt(tmp_path / "c.pth.tar", 0, 2.0)
    _ckpt(tmp_path / "c_best_loss.pth.tar", 0, 1.0)
    before = (tmp_path / "c_best_loss.pth.tar").stat().st_mtime_ns
    assert folder_loop.resume_position(resume, tmp_path / "c.pth.tar", tmp_path / "c_best_loss.pth.tar", True) == (1, 1.0)
    assert (tmp_path / "c_best_loss.pth.tar").stat().st_mtime_ns == before


def test_homography_train_takes_the_same_helper():
    assert homography_train.resume_position is folder_loop.resume_position       # called with copy_best=True: that command always saves


# ------------------------------------------------------------------------------------------------------------------------ the driver
RECORD_KEYS = ["epoch", "steps", "seconds_per_step", "best", "train", "valid", "train_loss", "valid_loss", "left_out_no_sidecar",
               "dropped_tail", "invalid_homographies"]


def _drive(mod, tmp_path, extra, losses, resume=None):
    a = mod.parser().parse_args(["root", "--patch-size", "64", "64", "--batch-size", "2", "--test-batch-size", "2", "--out", str(tmp_path),
                                 *extra])
    folder = SimpleNamespace(device=torch.device("cpu"), tcache=_Cache(), vcache=_Cache(SIZES[:2]), keep_t=[0, 1, 2, 4], keep_v=[0, 1],
                             resume=resume, seed=0)
    saved, logs, plans = [], [], []

    def train_pass(plan, homography):
        plans.append(plan)
        assert homography is None
        return {"loss": 7.0}, len(plan), 0.5 * len(plan)

    def valid_pass(plan, homography):
        return {"loss": losses[len(plans) - 1], "batches": len(plan)}

    def save(path, loss, epoch):
        saved.append((path.name, loss, epoch))
        torch.save({"epoch": epoch, "loss": loss}, path)

    stem = {train_folder: "checkpoint", train_stage2: "second_checkpoint"}[mod]
    hist = folder_loop.run_epochs(a, folder, stem, train_pass, valid_pass, save, logs.append)
    return hist, logs, saved, plans, stem


@pytest.mark.parametrize("mod", COMMANDS, ids=IDS)
def test_driver_records_best_and_files_over_three_epochs(mod, tmp_path):
    import json
    extra = ["--checkpoint", "synthetic"] if mod is train_stage2 else []
    hist, logs, saved, plans, stem = _drive(mod, tmp_path, [*extra, "-e", "3", "--save"], [3.0, 1.0, 2.0])
    assert [list(r) for r in hist] == [RECORD_KEYS + ["decode_seconds"], RECORD_KEYS, RECORD_KEYS]
    assert [json.loads(s) for s in logs] == hist
    assert [r["best"] for r in hist] == [True, True, False] and [r["epoch"] for r in hist] == [0, 1, 2]
    assert [r["valid_loss"] for r in hist] == [3.0, 1.0, 2.0] and [r["train_loss"] for r in hist] == [7.0] * 3
    assert hist[0]["steps"] == 2 and hist[0]["seconds_per_step"] == 0.5 and hist[0]["decode_seconds"] == 0.5
    assert hist[0]["left_out_no_sidecar"] == 1 and hist[0]["dropped_tail"] == 0 and hist[0]["invalid_homographies"] == 0
    assert saved == [(f"{stem}.pth.tar", 3.0, 0), (f"{stem}.pth.tar", 1.0, 1), (f"{stem}.pth.tar", 2.0, 2)]
    assert torch.load(tmp_path / f"{stem}.pth.tar") == {"epoch": 2, "loss": 2.0}
    assert torch.load(tmp_path / f"{stem}_best_loss.pth.tar") == {"epoch": 1, "loss": 1.0}
    assert sorted(f.name for f in tmp_path.iterdir()) == [f"{stem}.pth.tar", f"{stem}_best_loss.pth.tar"]
    assert [p.flags for p in plans] == [[[0, 0], [0, 0]]] * 3                    # no --augment: the plans carry zeros


@pytest.mark.parametrize("mod", COMMANDS, ids=IDS)
def test_driver_augment_graphed_resume_and_no_save(mod, tmp_path):
    extra = ["--checkpoint", "synthetic"] if mod is train_stage2 else []
    stem = {train_folder: "checkpoint", train_stage2: "second_checkpoint"}[mod]
    resume = _ckpt(tmp_path / "old" / f"{stem}.pth.tar", 0, 2.5)
    hist, _, saved, plans, _ = _drive(mod, tmp_path, [*extra, "-e", "3", "--augment", "hflip", "swap", "--graphed", "--batch-size", "3", "--resume",
                                                      str(tmp_path / "old" / f"{stem}.pth.tar")], [3.0, 2.0], resume)
    assert [list(r) for r in hist] == [RECORD_KEYS + ["augmented", "decode_seconds"], RECORD_KEYS + ["augmented"]]
    assert [r["epoch"] for r in hist] == [1, 2] and [r["best"] for r in hist] == [False, True]         # the resumed loss 2.5 counts
    assert hist[0]["dropped_tail"] == 1 and hist[0]["steps"] == 1
    assert hist[0]["augmented"] == plans[0].augmented() and list(hist[0]["augmented"]) == ["hflip", "vflip", "swap"]
    assert hist[0]["augmented"]["vflip"] == 0
    assert saved == [] and sorted(f.name for f in tmp_path.iterdir()) == ["old"]                        # no --save: nothing written


# ----------------------------------------------------------------------------------------------------------------------- the parsers
# dest -> (default, type, choices, nargs), as both commands declared them
SHARED_OPTIONS = {
    "root": (None, None, None, None),
    "epochs": (100, int, None, None),
    "learning_rate": (1e-4, float, None, None),
    "lmbda": (1e-2, float, None, None),
    "batch_size": (16, int, None, None),
    "test_batch_size": (64, int, None, None),
    "patch_size": ((256, 256), int, None, 2),
    "num_workers": (3, int, None, None),
    "save": (False, None, None, 0),
    "seed": (None, int, None, None),
    "homography": ("sidecar", None, ("sidecar", "net", "surf"), None),
    "homography_checkpoint": (None, None, None, None),
    "clip_max_norm": (None, float, None, None),
    "skip_nonfinite": (False, None, None, 0),
    "graphed": (False, None, None, 0),
    "dtype": ("bf16", None, ["bf16", "f32"], None),
    "cache": ("device", None, ("device", "stream"), None),
    "cache_gb": (None, float, None, None),
    "augment": ((), None, ("hflip", "vflip", "swap"), "+"),
    "valid_split": ("test", None, None, None),
    "out": (".", None, None, None),
    "model": ("hesic", None, ("hesic", "joint"), None),
    "resume": ("none", None, None, None),
}
OPTION_STRINGS = {"epochs": ["-e", "--epochs"], "learning_rate": ["-lr", "--learning-rate"], "lmbda": ["--lambda"],
                  "num_workers": ["-n", "--num-workers"]}


@pytest.mark.parametrize("mod", COMMANDS, ids=IDS)
def test_parsers_declare_the_shared_options_alike(mod):
    acts = {x.dest: x for x in mod.parser()._actions}
    for dest, want in SHARED_OPTIONS.items():
        x = acts[dest]
        assert (x.default, x.type, x.choices, x.nargs) == want, dest
        if dest != "root":
            assert x.option_strings == OPTION_STRINGS.get(dest, ["--" + dest.replace("_", "-")]), dest
    own = {train_folder: {"aux_learning_rate", "distortion"}, train_stage2: {"checkpoint", "infer_dtype"}}[mod]
    assert set(acts) - {"help"} == set(SHARED_OPTIONS) | own


def test_stage2_still_refuses_what_only_train_folder_takes(capsys):
    for bad in (["r", "--aux-learning-rate", "1"], ["r", "--distortion", "mse"], ["r", "--dtype", "f16"]):
        with pytest.raises(SystemExit) as e:
            train_stage2.parser().parse_args(bad)
        assert e.value.code == 2
    a = train_folder.parser().parse_args(["r", "--aux-learning-rate", "1", "--distortion", "ms-ssim"])
    assert (a.aux_learning_rate, a.distortion) == (1.0, "ms-ssim")


REFUSALS = [(["--patch-size", "64", "80"], "--patch-size must be positive multiples of 64, got 64 80"),
            (["--batch-size", "0"], "--batch-size, --test-batch-size and --num-workers must be positive and --epochs not negative"),
            (["-e", "-1"], "--batch-size, --test-batch-size and --num-workers must be positive and --epochs not negative"),
            (["--homography-checkpoint", "x.pth.tar"], "--homography-checkpoint needs --homography net"),
            (["--cache-gb", "0"], "--cache-gb must be positive"),
            # the first of several, in the order the commands always checked them
            (["--cache-gb", "0", "--homography-checkpoint", "x", "-n", "0"],
             "--batch-size, --test-batch-size and --num-workers must be positive and --epochs not negative")]


@pytest.mark.parametrize("mod", COMMANDS, ids=IDS)
@pytest.mark.parametrize("bad,message", REFUSALS, ids=[" ".join(b) for b, _ in REFUSALS])
def test_shared_refusals_exit_2_with_their_wording(mod, bad, message, tmp_path, capsys):
    # no folder is needed: the refusals come before the listing pass
    extra = ["--checkpoint", "synthetic"] if mod is train_stage2 else []
    with pytest.raises(SystemExit) as e:
        mod.main([str(tmp_path / "nowhere"), *extra, "--patch-size", "64", "64", *bad], log=lambda s: None)
    assert e.value.code == 2
    assert capsys.readouterr().err.rstrip().endswith("error: " + message)


def test_stage2s_own_refusal_comes_after_the_shared_ones_and_before_the_listing(tmp_path, capsys):
    with pytest.raises(SystemExit):
        train_stage2.main([str(tmp_path / "nowhere"), "--cache-gb", "0"], log=lambda s: None)
    assert "--cache-gb must be positive" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        train_stage2.main([str(tmp_path / "nowhere")], log=lambda s: None)
    assert e.value.code == 2
    assert capsys.readouterr().err.rstrip().endswith("--checkpoint is required: the frozen model's weights, or 'synthetic' for the deterministic ones")


# --------------------------------------------------------------------------------------------------------- the step controls' validation
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin, self.q = torch.nn.Linear(2, 2), torch.nn.Parameter(torch.zeros(3))

    def parameters(self, recurse=True):
        return self.lin.parameters()

    def aux_parameters(self):
        return [self.q]


def _make(name, **kw):
    if name == "Trainer":
        return train.GraphedTrainer(_Net(), **kw)            # ``Trainer``'s constructor, then the device check of the graphed class
    if name == "HomographyTrainer":
        return train.HomographyTrainer(_Net(), **kw)
    return train.EnhancerTrainer(_Net(), _Net(), **kw)


CLASSES = ["Trainer", "HomographyTrainer", "EnhancerTrainer"]


@pytest.mark.parametrize("name", CLASSES)
@pytest.mark.parametrize("bad", [0, -1, float("inf"), float("nan"), True, "1"], ids=repr)
def test_a_bad_clip_max_norm_is_refused_before_the_device_check(name, bad):
    with pytest.raises(ValueError) as e:
        _make(name, clip_max_norm=bad)
    assert str(e.value) == f"{name}: clip_max_norm must be a finite positive number (or None: no clipping), got {bad!r}"


@pytest.mark.parametrize("name", CLASSES)
@pytest.mark.parametrize("flag", ["skip_nonfinite", "live_lr"])
def test_a_flag_that_is_no_bool_is_refused_before_the_device_check(name, flag):
    with pytest.raises(TypeError) as e:
        _make(name, **{flag: 1})
    assert str(e.value) == f"{name}: {flag} must be a bool, got int"


@pytest.mark.parametrize("name", CLASSES)
def test_good_controls_reach_the_device_check_on_a_host_module(name):
    with pytest.raises(RuntimeError, match="ROCm device"):
        _make(name, clip_max_norm=1, skip_nonfinite=True, live_lr=True)
    assert train._step_controls(name, 2, False, True) == (2.0, False, True)
    assert isinstance(train._step_controls(name, 2, False, True)[0], float)
    assert train._step_controls(name, None, False, False) == (None, False, False)
