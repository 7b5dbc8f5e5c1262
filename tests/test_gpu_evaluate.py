"""model.evaluate() and `train.py --evaluate` on the GPU: the per-image metrics of every eval_pairs() entry agree with
metrics.image_metrics_host on the tensors each forward pass left, under the tolerance rule of tests/test_gpu_metrics.py; the
evaluation changes no state; the driver writes eval_<name>.json and, with --event_log, an event file holding the same scalars."""
import glob
import json
import math
import os

import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import metrics, summary
from dynamic_multiview_3d_amd.train import SyntheticData

pytestmark = pytest.mark.gpu

BATCH, NBATCH = 4, 3


def _build(name, seed=1234):
    if name == 'appflow':
        from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
        return AppearanceFlowModel({'batch_size': BATCH, 'learning_rate': 1e-4}, load_tfrec=False, device='cuda', seed=seed)
    from dynamic_multiview_3d_amd import mv3d
    return mv3d.mv3d_nobg_dm({'batch_size': BATCH}, device='cuda', seed=seed)


def _state_bits(model):
    model.graph.settle()
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy().copy() for k, v in model.graph.state_dict().items()}


@pytest.mark.parametrize("name", ['appflow', 'mv3d_nobg_dm'])
def test_evaluate_equals_the_host_metrics_of_each_forward(name):
    model = _build(name)
    for _ in range(2):                                           # a model that has trained a little: gen is not trivial
        model.train_step(**SyntheticData(model, seed=7).next())
    before = _state_bits(model)
    res = model.evaluate(SyntheticData(model), NBATCH)
    after = _state_bits(model)
    assert before.keys() == after.keys()
    for k in before:
        assert before[k].dtype == after[k].dtype and before[k].tobytes() == after[k].tobytes(), k

    pairs = model.eval_pairs()
    assert [p[0] for p in pairs] == (['image'] if name == 'appflow' else ['image', 'depth'])
    data = SyntheticData(model)                                  # the same seed: the same three batches
    losses, h64, h32 = [], {p[0]: [] for p in pairs}, {p[0]: [] for p in pairs}
    for _ in range(NBATCH):
        losses.append(float(model.forward(**data.next())))
        for pname, pred, target, max_val in pairs:
            p, t = pred.numpy(), target.numpy()
            h64[pname].append(metrics.image_metrics_host(p, t, max_val, np.float64))
            h32[pname].append(metrics.image_metrics_host(p, t, max_val, np.float32).astype(np.float64))
    assert res['images'] == BATCH * NBATCH
    print(name, res)
    assert abs(res['loss'] - np.mean(losses)) <= 1e-6 * abs(np.mean(losses))          # fp32 losses averaged in double
    for pname, _, _, max_val in pairs:
        a64, a32 = np.concatenate(h64[pname]), np.concatenate(h32[pname])
        # the rule of test_gpu_metrics.py on the means over the images: 4 x the float32 gap, floors 2e-6 relative (l1, mse) and
        # 2e-6 absolute (ssim); psnr = 10 log10(max_val^2 / mse), so a relative mse error r moves it by 10 / ln(10) * r dB
        gap = np.abs(a32 - a64)
        rel_mse = np.maximum(4 * gap[:, 1] / a64[:, 1], 2e-6)
        want = {'l1': (a64[:, 0].mean(), max(4 * gap[:, 0].mean(), 2e-6 * a64[:, 0].mean())),
                'ssim': (a64[:, 2].mean(), max(4 * gap[:, 2].mean(), 2e-6)),
                'psnr': (metrics.psnr(a64[:, 1], max_val).mean(), 10 / math.log(10) * rel_mse.mean())}
        for key, (value, allowed) in want.items():
            got = res['%s/%s' % (pname, key)]
            print('%s %s/%s evaluate %.9g host %.9g |diff| %.2e allowed %.2e' % (name, pname, key, got, value, abs(got - value), allowed))
            assert abs(got - value) <= allowed, (pname, key, got, value, allowed)
        assert res[pname + '/l1'] >= 0 and res[pname + '/ssim'] <= 1


def test_train_step_after_evaluate_gives_the_same_loss_bits():
    def run(with_eval):
        model = _build('appflow')
        data = SyntheticData(model, seed=3)
        model.train_step(**data.next())
        if with_eval:
            model.evaluate(SyntheticData(model, seed=11), 2)
        loss = model.train_step(**data.next())
        return np.float32(float(loss)).view(np.uint32), _state_bits(model)
    (l0, s0), (l1, s1) = run(False), run(True)
    assert l0 == l1
    for k in s0:
        assert s0[k].tobytes() == s1[k].tobytes(), k


def _conf(tmp_path):
    conf_py = tmp_path / 'conf.py'
    conf_py.write_text(
        "import os\nfrom lowdim_angle import AppFlowLowDimAngle\n"
        "configuration = {'experiment_name': 't', 'data_dir': '', 'output_dir': os.path.dirname(os.path.realpath(__file__)) + '/modeldata',\n"
        "  'num_iterations': 2, 'batch_size': 2, 'learning_rate': 1e-4, 'train_val_split': 0.95, 'model': AppFlowLowDimAngle}\n")
    return str(conf_py), tmp_path / 'modeldata'


def test_train_driver_evaluates_a_checkpoint_and_logs_events(tmp_path):
    from dynamic_multiview_3d_amd import train
    conf, out = _conf(tmp_path)
    train.main(['--hyper', conf, '--synthetic'])
    assert (out / 'model.index').exists()
    assert glob.glob(str(out / 'events.out.tfevents*')) == []             # no --event_log: nothing new is written
    for ext in ('.index', '.data-00000-of-00001'):
        os.replace(str(out / 'model') + ext, str(out / 'model2') + ext)   # a name that carries its iteration
    train.main(['--hyper', conf, '--synthetic', '--evaluate', 'model2', '--eval_batches', '2', '--event_log'])
    res = json.load(open(out / 'eval_model2.json'))
    assert res['images'] == 4 and res['iteration'] == 2 and res['checkpoint'] == 'model2'
    assert math.isfinite(res['loss']) and res['image/l1'] >= 0 and res['image/ssim'] <= 1 and res['image/psnr'] > 0
    files = glob.glob(str(out / 'events.out.tfevents*'))
    assert len(files) == 1
    events = summary.read_events(files[0])
    assert events[0]['file_version'] == 'brain.Event:2'
    scalars = {}
    for e in events[1:]:
        assert e['step'] == 2
        scalars.update(dict(e['scalars']))
    assert set(scalars) == {'test_loss', 'image/l1', 'image/psnr', 'image/ssim'}
    assert scalars['test_loss'] == float(np.float32(res['loss']))
    for key in ('image/l1', 'image/psnr', 'image/ssim'):
        assert scalars[key] == float(np.float32(res[key]))


def test_train_driver_event_log_holds_the_training_loss(tmp_path):
    from dynamic_multiview_3d_amd import train
    conf, out = _conf(tmp_path)
    train.main(['--hyper', conf, '--synthetic', '--event_log'])
    rows = [json.loads(l) for l in open(out / 'train_log.jsonl')]
    files = glob.glob(str(out / 'events.out.tfevents*'))
    assert len(files) == 1
    got = [(e['step'], e['scalars'][0]) for e in summary.read_events(files[0])[1:]]
    assert got == [(r['itr'], ('training_loss', float(np.float32(r['training_loss'])))) for r in rows if 'training_loss' in r]
