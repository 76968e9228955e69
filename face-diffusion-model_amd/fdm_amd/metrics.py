"""On-device evaluation metrics of the reference: lip / face vertex error,
mean vertex error, emotion mean error, upper-face dynamics deviation (FDD) and diversity.

Mirrors computer_metrix.py:6-136 (BIWI / VOCASET evaluation, `main`), :139-194 (`compute_diversity`) and the
vertex-error block of metric/metric.py:115-138 (3D-MEAD; its ground truth comes from FLAME parameters: pass
gt_params= and a flame.FlamePlan made from the user's model file, or vertex arrays).  The reductions run in
libfdm_hip.so (fdm_op_vertex_err, fdm_op_motion_std); numpy/pickle are used for file IO only."""
import argparse
import os
import pickle

import numpy as np
import torch

from . import ops
from ._lib import FdmError


def _dev(a, device, dtype=torch.float32):
    t = torch.as_tensor(np.ascontiguousarray(a)) if not torch.is_tensor(a) else a
    return t.to(device=device, dtype=dtype).contiguous()


def _region(region, V, device):
    if region is None:
        return None, V
    r = _dev(np.asarray(region, dtype=np.int64), device, torch.int32)
    if r.numel() == 0 or int(r.min()) < 0 or int(r.max()) >= V:
        raise FdmError("vertex region is empty or out of range")
    return r, r.numel()


def vertex_error(gt, pred, region=None, device="cuda:0"):
    """gt, pred [F, V, 3] -> dict(max=mean_f max_r d2, mean_sq=mean d2, mean_dist=mean |d|, frame_max=[F] tensor),
    d2 = |gt - pred|^2 over the region's vertices (all vertices when region is None)."""
    g, p = _dev(gt, device), _dev(pred, device)
    if g.shape != p.shape or g.dim() != 3 or g.shape[2] != 3:
        raise FdmError(f"vertex_error expects two [F, V, 3] arrays, got {tuple(g.shape)} and {tuple(p.shape)}")
    F, V = g.shape[0], g.shape[1]
    r, R = _region(region, V, device)
    fmax = torch.empty(F, device=device)
    fsum = torch.empty(2 * F, device=device, dtype=torch.float64)
    out = torch.empty(3, device=device, dtype=torch.float64)
    ops.vertex_err(g, p, r, R, F, V, fmax, fsum, out)
    o = out.cpu()
    return dict(max=float(o[0]), mean_sq=float(o[1]), mean_dist=float(o[2]), frame_max=fmax)


def motion_std(verts, template, region, device="cuda:0"):
    """mean over the region of the per-vertex std over frames of |verts - template|^2 (computer_metrix.py:95-105)."""
    v = _dev(verts, device)
    F, V = v.shape[0], v.shape[1]
    t = _dev(np.asarray(template).reshape(-1, 3) if not torch.is_tensor(template) else template.reshape(-1, 3), device)
    if t.shape[0] != V:
        raise FdmError(f"template has {t.shape[0]} vertices, sequence has {V}")
    r, R = _region(region, V, device)
    partial = torch.empty(2 * min(F, 64) * R, device=device, dtype=torch.float64)
    out = torch.empty(1, device=device, dtype=torch.float64)
    ops.motion_std(v, t, r, R, F, V, partial, out)
    return float(out.cpu()[0])


def lip_vertex_error(gt, pred, mouth_map, device="cuda:0"):
    """'Lip Vertex Error' (computer_metrix.py:121-127): mean over frames of the max squared lip-vertex error."""
    return vertex_error(gt, pred, mouth_map, device)["max"]


def mean_vertex_error(gt, pred, device="cuda:0"):
    """'Mean Vertex Error' (computer_metrix.py:118-119)."""
    return vertex_error(gt, pred, None, device)["mean_dist"]


def upper_face_dynamics_deviation(gt, pred, template, upper_map, device="cuda:0"):
    """Per-sequence FDD term (computer_metrix.py:95-107): std-of-motion(gt) - std-of-motion(pred)."""
    return motion_std(gt, template, upper_map, device) - motion_std(pred, template, upper_map, device)


def load_regions(region_path, dataset):
    """Vertex index lists as computer_metrix.py:23-55 reads them."""
    if dataset == "BIWI":
        with open(os.path.join(region_path, "lve.txt")) as f:
            mouth = [int(i) for i in f.read().split(", ")]
        with open(os.path.join(region_path, "fdd.txt")) as f:
            upper = [int(i) for i in f.read().split(", ")]
        return mouth, upper, 23370, ["e" + str(i).zfill(2) for i in range(37, 41)]
    with open(os.path.join(region_path, "weighted_mouth_mask.txt")) as f:
        mouth = [i for i, v in enumerate(float(line.strip()) for line in f if line) if v > 0.1]
    with open(os.path.join(region_path, "forehead_mask.txt")) as f:
        upper = [i for i, v in enumerate(float(line.strip()) for line in f if line) if v > 0.4]
    return mouth, upper, 6172, [str(i) for i in range(46, 51)]


def pred_name(subject, sentence, condition=None, model=""):
    """Basename of a prediction file as computer_metrix.py reads it: `<subject>_<sentence>` (:74, what the MEAD / BIWI samplers
    write), `<subject>_<sentence>_condition_<conditioning subject>` (:171-174, what samples/sample_diffusion_vocaset.py:86-88
    writes), with `<model>_` in front when a model tag is given (:69-71)."""
    name = subject + "_" + sentence + (("_condition_" + condition) if condition is not None else "")
    return (model + "_" + name) if model != "" else name


def evaluate(pred_path, gt_path, region_path, templates_path, train_subjects="F2 F3 F4 M3 M4 M5", model="", dataset="BIWI",
             device="cuda:0", verbose=True):
    """computer_metrix.py `main` (:6-136): same files, same naming, same printed lines; returns the numbers."""
    mouth, upper, nv, sentences = load_regions(region_path, dataset)
    with open(templates_path, "rb") as fin:
        templates = pickle.load(fin, encoding="latin1")
    say = print if verbose else (lambda *a, **k: None)
    gts, preds, fdd = [], [], []
    for subject in train_subjects.split(" "):
        for sentence in sentences:
            gt = np.load(os.path.join(gt_path, subject + "_" + sentence + ".npy")).reshape(-1, nv, 3)
            name = pred_name(subject, sentence, subject, model) if model != "" else pred_name(subject, sentence)
            pred = np.load(os.path.join(pred_path, name + ".npy")).reshape(-1, nv, 3)
            n = min(gt.shape[0], pred.shape[0])
            gt, pred = _dev(gt[:n], device), _dev(pred[:n], device)
            say(tuple(pred.shape))
            fdd.append(upper_face_dynamics_deviation(gt, pred, templates[subject], upper, device))
            say(f"{subject}_{sentence}")
            say("FDD: {:.4e}".format(fdd[-1]), "FDD: {:.4e}".format(sum(fdd) / len(fdd)))
            gts.append(gt)
            preds.append(pred)
    gt_all, pred_all = torch.cat(gts), torch.cat(preds)
    say("Frame Number: {}".format(gt_all.shape[0]))
    say(tuple(gt_all.shape))
    res = dict(frames=int(gt_all.shape[0]),
               mean_vertex_error=vertex_error(gt_all, pred_all, None, device)["mean_dist"],
               lip_vertex_error=vertex_error(gt_all, pred_all, mouth, device)["max"],
               fdd=sum(fdd) / len(fdd), abs_fdd=sum(abs(x) for x in fdd) / len(fdd))
    say("Mean Vertex Error: {:.4e}".format(res["mean_vertex_error"]))
    say("Lip Vertex Error: {:.4e}".format(res["lip_vertex_error"]))
    say("FDD: {:.4e}".format(res["fdd"]))
    say("ABS FDD: {:.4e}".format(res["abs_fdd"]))
    return res


def diversity(pred_path, train_subjects, test_subjects, dataset="BIWI", device="cuda:0", verbose=True, sentences=None, nr_vertices=None):
    """computer_metrix.py `compute_diversity` (:139-194): mean pairwise vertex distance between the predictions of one
    test sequence under different conditioning subjects.  `sentences` / `nr_vertices` override the two tables the reference
    hard-codes per dataset (:155-162), e.g. VOCASET's 5023-vertex meshes and `sentenceNN` names."""
    nv = nr_vertices or (23370 if dataset == "BIWI" else 6172)
    sentences = sentences or (["e" + str(i).zfill(2) for i in range(37, 41)] if dataset == "BIWI" else [str(i) for i in range(46, 51)])
    say = print if verbose else (lambda *a, **k: None)
    total, num = 0.0, 0
    for subject in test_subjects.split(" "):
        for sentence in sentences:
            say(subject, sentence)
            seqs = []
            for cond in train_subjects.split(" "):
                fp = os.path.join(pred_path, pred_name(subject, sentence, cond) + ".npy")
                if os.path.exists(fp):
                    seqs.append(_dev(np.load(fp).reshape(-1, nv, 3), device))
            n = len(seqs)
            if n < 2:
                continue
            d = 0.0
            for i in range(n - 1):
                for j in range(i + 1, n):
                    d += vertex_error(seqs[i], seqs[j], None, device)["mean_dist"]
            d /= (n - 1) * n / 2
            say(d)
            total += d
            num += 1
    if num == 0:
        raise FdmError("diversity: no test sequence has two or more conditioned predictions")
    say("Diversity: {:.4e}".format(total / num))
    return total / num


def mead_vertex_metrics(gt, pred, face_vertex, lip_vertex, emotion_vertex, device="cuda:0", gt_params=None, flame=None):
    """The vertex-error block of metric/metric.py:115-138 on [F, 5023, 3] arrays: FVE, LVE (max over the region),
    EME (mean over the region) and the all-vertex error.  gt_params = (expression [F, NE], pose [F, 6]) with flame = a
    flame.FlamePlan, in place of gt (pass gt=None): the ground truth is made on the device as the reference makes it
    (flame.torch2mesh: zero shape, zero neck and eyes, 4 decimals)."""
    if gt_params is not None:
        if gt is not None or flame is None:
            raise ValueError("gt_params takes flame= (a flame.FlamePlan) and gt=None")
        from .flame import torch2mesh
        gt = torch2mesh(flame, gt_params[0], gt_params[1]).reshape(-1, flame.V, 3)
    return dict(FVE=vertex_error(gt, pred, face_vertex, device)["max"], LVE=vertex_error(gt, pred, lip_vertex, device)["max"],
                EME=vertex_error(gt, pred, emotion_vertex, device)["mean_sq"], ALL=vertex_error(gt, pred, None, device)["max"])


MEAD_REGIONS = ("face_vertices.npy", "lip_vertices.npy", "emotion_vertices.npy")


def mead_gt_name(pred):
    """(subject directory, ground-truth file) of a MEAD prediction file, the naming rule of metric/metric.py:67-70: the name with
    '_' turned into '-', cut before its last 10 characters, then '_', the 5 characters before the extension, '.npz'."""
    s = pred.replace("_", "-")
    return pred.split("_")[0], s[:-10] + "_" + s[-9:-4] + ".npz"


def mead_evaluate(pred_path, gt_path, flame_model, region_path="region", device="cuda:0", pick="angry", expr_at=None, verbose=True):
    """metric/metric.py:63-138 with the ground truth and the neutral template made on the device from FLAME parameters.  For every
    prediction <pred_path>/*.npy whose name holds `pick` (None: all) and whose ground truth <gt_path>/<subject>/<name>.npz (keys
    expression [T, NE], pose [T, 6]) exists: gt = torch2mesh(expression, (0, jaw pose)) -- the global rotation is dropped, as the
    reference drops it --, both cut to the shorter; then FVE / LVE / EME / ALL over all kept frames (mead_vertex_metrics) with the
    regions <region_path>/{face,lip,emotion}_vertices.npy, and per file the motion statistic of the emotion region about the neutral
    template (motion_std) for ground truth and prediction.  flame_model: a model file, a flame.FlameModel or a flame.FlamePlan.
    -> dict(FVE, LVE, EME, ALL, frames, files, motion_std_gt, motion_std_pred, template [V, 3])."""
    from .flame import FlameModel, FlamePlan, torch2mesh
    if isinstance(flame_model, FlamePlan):
        plan = flame_model
    else:
        plan = FlamePlan(flame_model if isinstance(flame_model, FlameModel) else FlameModel.load(flame_model, expr_at=expr_at), device=device)
    face, lip, emotion = (np.load(os.path.join(region_path, f)) for f in MEAD_REGIONS)
    V = plan.V
    n_expr = plan.NB - plan.model.expr_at
    template = torch2mesh(plan, torch.zeros(1, min(50, n_expr)), torch.zeros(1, 6)).reshape(V, 3)
    gts, preds, files, std_gt, std_pred = [], [], [], [], []
    for pred in sorted(os.listdir(pred_path)):
        if not pred.endswith(".npy") or (pick and pick not in pred):
            continue
        sub, name = mead_gt_name(pred)
        src = os.path.join(gt_path, sub, name)
        if not os.path.exists(src):
            if verbose:
                print(f"{pred}: ground truth {src} not found")
            continue
        with np.load(src) as z:
            ex, jaw = torch.from_numpy(z["expression"].astype(np.float32)), torch.from_numpy(z["pose"].astype(np.float32))[:, 3:6]
        vp = torch.from_numpy(np.load(os.path.join(pred_path, pred)).astype(np.float32).reshape(-1, V, 3)).to(device)
        vg = torch2mesh(plan, ex[:, :n_expr], torch.cat([torch.zeros_like(jaw), jaw], 1)).reshape(-1, V, 3)
        n = min(vp.shape[0], vg.shape[0])
        vp, vg = vp[:n].contiguous(), vg[:n].contiguous()
        gts.append(vg)
        preds.append(vp)
        files.append(pred)
        std_gt.append(motion_std(vg, template, emotion, device))
        std_pred.append(motion_std(vp, template, emotion, device))
    if not files:
        raise FdmError(f"no prediction in {pred_path} has a ground truth under {gt_path}")
    res = mead_vertex_metrics(torch.cat(gts), torch.cat(preds), face, lip, emotion, device)
    res.update(frames=int(sum(g.shape[0] for g in gts)), files=files, motion_std_gt=std_gt, motion_std_pred=std_pred, template=template)
    if verbose:
        print(f"Frame Number: {res['frames']}")
        print(f"Face Vertex Error (FVE): {res['FVE']:.4e}\nLip Vertex Error (LVE): {res['LVE']:.4e}")
        print(f"Emotion Mean Error (EME): {res['EME']:.4e}\nAll Vertex Error: {res['ALL']:.4e}")
    return res


def mead_main(argv=None):
    """CLI of metric/metric.py (:19-24) plus --flame_model: the model file the ground truth is made with."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--train_subjects", type=str, default="F2 F3 F4 M3 M4 M5")
    ap.add_argument("--pred_path", type=str, default="result/npy")
    ap.add_argument("--gt_path", type=str, default="MEAD/FLAME_ALL")
    ap.add_argument("--region_path", type=str, default="region")
    ap.add_argument("--templates_path", type=str, default="BIWI/templates.pkl")
    ap.add_argument("--flame_model", type=str, required=True,
                    help="build-added: FLAME-type model file (.npz or a pickled dict of plain arrays): ground truth and neutral template on the device")
    ap.add_argument("--flame_expr_at", type=int, default=None, help="build-added: index of the first expression coefficient (FLAME: 300)")
    ap.add_argument("--pick", type=str, default="angry", help="build-added: substring a prediction's name must hold (the reference's 'angry'; '' = all)")
    ap.add_argument("--device", type=str, default="cuda:0")
    a = ap.parse_args(argv)
    return mead_evaluate(a.pred_path, a.gt_path, a.flame_model, a.region_path, a.device, a.pick or None, a.flame_expr_at)


def main(argv=None):
    """CLI of computer_metrix.py (:7-17 and :140-150), then `main()` and `compute_diversity()` as its __main__ does."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--train_subjects", type=str, default="F2 F3 F4 M3 M4 M5")
    ap.add_argument("--test_subjects", type=str, default="F1 F5 F6 F7 F8 M1 M2 M6")
    ap.add_argument("--pred_path", type=str, default="/data/WX/fdm/checkpoints/diffusion_Encoder_Decoder/result")
    ap.add_argument("--gt_path", type=str, default="/data/WX/BIWI_dataset/vertices_npy")
    ap.add_argument("--region_path", type=str, default="/data/WX/BIWI_dataset/regions/")
    ap.add_argument("--templates_path", type=str, default="/data/WX/BIWI_dataset/templates.pkl")
    ap.add_argument("--model", type=str, default="")
    ap.add_argument("--num_sample", type=str)
    ap.add_argument("--dataset", type=str, default="BIWI")
    ap.add_argument("--device", type=str, default="cuda:0")
    a = ap.parse_args(argv)
    evaluate(a.pred_path, a.gt_path, a.region_path, a.templates_path, a.train_subjects, a.model, a.dataset, a.device)
    try:
        diversity(a.pred_path, a.train_subjects, a.test_subjects, a.dataset, a.device)
    except FdmError as e:
        print(e)
