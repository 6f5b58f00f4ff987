"""evaluate() and what it is made of, on the MI355X: the pose-metrics kernel, the four protocols, and run_evaluation() /
run_evaluation_3dhp()."""
import pytest
import torch

from conftest import gold
from helpers import inputs, product

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ the four protocols
def test_pose_metrics_kernel_against_the_reference_values():
    """d3d_pose_metrics (evaluate()'s P-MPJPE / N-MPJPE / MPJVE on the device, one thread per kept frame, fp64 inside, the 3 x 3 SVD by a
    Jacobi eigen-decomposition) against values of the reference's own functions (tests/golden/pose_metrics.npz): near / unrelated / mirrored
    (det R < 0) / planar (singular H) / mm-scale batches, the nan of a one-frame batch -- and the same batches with dropped frames spliced
    in (target_mask): the kept frames alone decide the values, the velocity differences run over consecutive KEPT frames (RUN:588-590)."""
    import numpy as np
    from diff3dhpe_amd.engine import pose_metrics
    g = gold("pose_metrics")
    rng = np.random.RandomState(3)
    for tag in g["tags"]:
        pr, tg, ref = g[f"{tag}_pred"], g[f"{tag}_gt"], g[f"{tag}_ref"]
        n = pr.shape[0]
        keep = np.ones(n + n // 3 + 2, dtype=bool)
        keep[rng.choice(len(keep), len(keep) - n, replace=False)] = False
        prm = rng.uniform(-5, 5, (len(keep), 17, 3)).astype(np.float32)
        tgm = rng.uniform(-5, 5, (len(keep), 17, 3)).astype(np.float32)
        prm[keep], tgm[keep] = pr, tg
        for P, G, M in ((pr, tg, None), (prm, tgm, keep)):
            kept, en, ep, ev = pose_metrics(torch.from_numpy(P).cuda(), torch.from_numpy(G).cuda(), None if M is None else torch.from_numpy(M).cuda())
            assert kept == n
            for name, got, want in (("p_mpjpe", ep, ref[1]), ("n_mpjpe", en, ref[2]), ("mpjve", ev, ref[3])):
                if np.isnan(want):
                    assert np.isnan(got), (tag, name, got)
                else:
                    assert abs(got - want) <= 2e-6 * abs(want) + 1e-7, (tag, name, got, want)     # (the reference computes these in fp32)


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
def test_evaluate_returns_the_four_protocols(prec):
    """evaluate() end to end (two DDIM samplings per window, merge, mask, the four running sums weighted by each batch's kept frames,
    RUN:562-614) against the oracle's sampler + its restatement of the reference's metric functions: two batches, one with masked frames,
    through as_reference_tuple() -- the reference's own return shape (e1, e2, e3, ev, N, epoch_time)."""
    from diff3dhpe_amd.evaluate import evaluate, as_reference_tuple, flip_2d, H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT
    from oracle import d3d_oracle as orc
    from helpers import cfg_small, hashed, torch_sd, build_product
    cfg = cfg_small(27)
    _, diff = build_product(cfg, 12, sampling=3, precision=prec)
    sd, tabs = torch_sd(cfg, 12), orc.diffusion_tables("cosine", 1000)
    kw = dict(num_timesteps=1000, sampling_timesteps=3, depth=cfg.depth)
    batches, tot, N = [], [0.0, 0.0, 0.0, 0.0], 0
    for b, (B, seed) in enumerate(((3, 101), (2, 202))):
        inp = inputs(B, 27, seed)
        mask = torch.ones(B, 27, dtype=torch.bool)
        if b == 0:
            mask[1, :11] = False
        nz_f = hashed(f"flipnoise{b}", tuple(inp["noise"].shape), 1)
        batches.append({"inputs_2d": inp["x2d"], "inputs_3d": inp["gt3d"], "target_mask": mask, "init_noise": inp["noise"], "init_noise_flip": nz_f})
        p = orc.ddim_sample_loop(sd, tabs, inp["x2d"], inp["noise"], **kw)
        pf = orc.ddim_sample_loop(sd, tabs, flip_2d(inp["x2d"], H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT), nz_f, **kw)
        merged = orc.merge_flip_tta(p, pf, 1.3, mask)
        gtm = inp["gt3d"].view(-1, 17, 3)[mask.view(-1)].unsqueeze(1)
        n, s1, s2, s3, sv = orc.protocol_sums(merged, gtm)
        N += n
        for i, v in enumerate((s1, s2, s3, sv)):
            tot[i] += v
    e1, e2, e3, ev, frames, secs = as_reference_tuple(evaluate(diff, batches, scale=1.3, verbose=False))
    assert frames == N and secs > 0
    for name, got, want in (("mpjpe", e1, tot[0]), ("p_mpjpe", e2, tot[1]), ("n_mpjpe", e3, tot[2]), ("mpjve", ev, tot[3])):
        assert abs(got - want / N * 1000) < 0.05, (name, got, want / N * 1000)      # mm at scale 1.3: 1e-4 of the sampler's gate and to spare
    only1 = evaluate(diff, batches, scale=1.3, verbose=False, all_protocols=False)
    assert only1["p_mpjpe_mm"] is None and abs(only1["mpjpe_mm"] - e1) < 1e-9


def test_run_evaluation_action_wise_averages():
    """run_evaluation() (RUN:712-766): one evaluate() per action name over the actions with that prefix, action-wise means of the four
    protocols, totals -- against the same evaluate() calls made by hand with the generator in the same state."""
    from diff3dhpe_amd.data import EvalData, MocapMeta
    from diff3dhpe_amd.evaluate import evaluate, run_evaluation, as_reference_tuple
    from diff3dhpe_amd.synth import synth_mocap, SYNTH_JOINTS_LEFT as JL, SYNTH_JOINTS_RIGHT as JR
    from helpers import cfg_small, build_product
    pos, cams, kp, meta = synth_mocap(0)
    ed = EvalData(MocapMeta(pos, cams, JL, JR), kp, meta["keypoints_symmetry"], ["S9", "S11"], 27)
    _, diff = build_product(cfg_small(27), 31, sampling=2, precision="f16x3")
    torch.manual_seed(5)
    torch.cuda.manual_seed(5)
    res = run_evaluation(diff, ed, batch_size=4, verbose=False)
    torch.manual_seed(5)
    torch.cuda.manual_seed(5)
    by_hand = {}
    for name in ed.action_names():
        by_hand[name] = as_reference_tuple(evaluate(diff, ed.batches(4, action_filter=[name]), scale=ed.scale, joints_left=ed.joints_left,
                                                    joints_right=ed.joints_right, verbose=False))
    assert list(res["actions"]) == ["Walk", "Sit", "Eat", "Wait"]
    for name, t in by_hand.items():
        assert res["actions"][name][:5] == t[:5], name
    for i, key in enumerate(("mpjpe_mm", "p_mpjpe_mm", "n_mpjpe_mm", "mpjve_mm")):
        assert abs(res[key] - sum(t[i] for t in by_hand.values()) / 4) < 1e-9
    assert res["frames"] == sum(t[4] for t in by_hand.values()) == sum(int(it["target_mask"].sum()) for it in ed.items())
    only = run_evaluation(diff, ed, batch_size=4, action_filter=["Wa"], verbose=False)
    assert list(only["actions"]) == ["Walk", "Wait"]


def test_run_evaluation_3dhp_per_sequence_and_stored_predictions(tmp_path):
    """run_evaluation_3dhp() (run_..._3dhp.py:593-632) with a seq2frame model on the synthetic 3DHP-shaped data set: one evaluate() per test
    sequence with forward()'s default output_loss, sequence-wise averages of the four protocols, and data_inference[seq] = the kept frames'
    merged predictions as (3, J, N) -- equal to what evaluate() computes by hand with the generator in the same state; inference_data.mat
    readable by scipy."""
    import numpy as np
    import scipy.io as scio
    from diff3dhpe_amd.data import EvalData3DHP
    from diff3dhpe_amd.evaluate import evaluate, run_evaluation_3dhp, as_reference_tuple
    from diff3dhpe_amd.synth import synth_mocap_3dhp
    from helpers import cfg_small
    test, train = synth_mocap_3dhp(0)
    ed = EvalData3DHP(test, ["TS1", "TS5"], 27, out_all=False, train_data=train)
    _, diff = product(cfg_small(27, seq2frame=True, with_time_emb=False), 9, "f16x3", sampling=2)
    mat = str(tmp_path / "inference_data.mat")
    torch.manual_seed(11)
    torch.cuda.manual_seed(11)
    res = run_evaluation_3dhp(diff, ed, batch_size=32, verbose=False, mat_path=mat)
    torch.manual_seed(11)
    torch.cuda.manual_seed(11)
    for name in ("TS1", "TS5"):
        r = evaluate(diff, ed.batches(32, seq_filter=name), scale=ed.scale, joints_left=ed.joints_left, joints_right=ed.joints_right,
                     verbose=False, unit_scale=1.0, output_loss=True, collect_predictions=True)
        assert res["sequences"][name][:5] == as_reference_tuple(r)[:5]
        valid = int(sum(int(it["target_mask"].sum()) for it in ed.items(seq_filter=name)))
        assert res["data_inference"][name].shape == (3, 17, valid) == tuple(r["predictions"].permute(2, 1, 0).shape)
        assert np.array_equal(res["data_inference"][name], r["predictions"].permute(2, 1, 0).numpy())
    for i, key in enumerate(("mpjpe_mm", "p_mpjpe_mm", "n_mpjpe_mm", "mpjve_mm")):
        assert abs(res[key] - (res["sequences"]["TS1"][i] + res["sequences"]["TS5"][i]) / 2) < 1e-9 and np.isfinite(res[key])
    m = scio.loadmat(mat)
    assert np.array_equal(m["TS1"], res["data_inference"]["TS1"]) and m["TS5"].shape[:2] == (3, 17)
