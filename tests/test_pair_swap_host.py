"""Pair-swapped batches without a GPU: the numpy mirror, the reader over a small shard written with the project's own writer (with
and without colour augmentation), the key's refusals, and the key-off batches."""
import numpy as np
import pytest
import torch

from dynamic_multiview_3d_amd import pair_swap as P
from dynamic_multiview_3d_amd import read_tf_records as R
from tests import color_augment_cases as CC

H = 16
B = 4
SHAPES = {'image0': (B, H, H, 3), 'image1': (B, H, H, 3), 'depth_image0': (B, H, H, 1), 'depth_image1': (B, H, H, 1), 'disp': (B, 2)}


def _records(h, seed=0):
    rng = np.random.default_rng(seed)
    out = {'image0': rng.uniform(0, 1, (h, H, H, 3)).astype(np.float32), 'image1': rng.uniform(0, 1, (h, H, H, 3)).astype(np.float32),
           'depth_image0': rng.uniform(0, 1, (h, H, H, 1)).astype(np.float32), 'depth_image1': rng.uniform(0, 1, (h, H, H, 1)).astype(np.float32),
           'disp': rng.uniform(-1, 1, (h, 2)).astype(np.float32)}
    out['disp'][0] = (0.0, -0.0)
    return out


def _check_layout(full, h):
    """The second half is the first read backwards, bit for bit."""
    for x, y in P.SWAPPED:
        assert np.asarray(full[x][h:]).tobytes() == np.asarray(full[y][:h]).tobytes(), x
        assert np.asarray(full[y][h:]).tobytes() == np.asarray(full[x][:h]).tobytes(), y
    assert np.asarray(full['disp'][h:]).tobytes() == np.negative(np.asarray(full['disp'][:h])).tobytes()


def test_mirror_host_lays_out_the_pairs_and_is_an_involution():
    rec = _records(3)
    full = P.mirror_host(rec)
    assert list(full) == list(rec) and all(v.shape[0] == 6 and v.dtype == np.float32 for v in full.values())
    for k in rec:
        assert full[k][:3].tobytes() == rec[k].tobytes(), k               # samples 0 .. B/2-1 are the records as read
    _check_layout(full, 3)
    assert np.signbit(full['disp'][3]).tolist() == [True, False]          # -(0.0) = -0.0 and -(-0.0) = 0.0
    # mirroring the reversed half gives the records back as ITS reverses
    again = P.mirror_host({k: v[3:] for k, v in full.items()})
    for k in rec:
        assert again[k][3:].tobytes() == rec[k].tobytes(), k
    with pytest.raises(ValueError, match='exactly the inputs'):
        P.mirror_host(dict(rec, image1_only0=rec['image0']))
    with pytest.raises(ValueError, match='exactly the inputs'):
        P.mirror_host({k: v for k, v in rec.items() if k != 'disp'})


def test_the_torch_stage_equals_the_numpy_statement():
    rec = _records(2, seed=1)
    stage = P.PairSwap({'batch_size': 4, 'pair_swap': True})
    got = stage.apply({k: torch.from_numpy(v) for k, v in rec.items()})
    want = P.mirror_host(rec)
    assert list(got) == list(rec)
    for k in rec:
        assert got[k].numpy().tobytes() == want[k].tobytes(), k
    with pytest.raises(ValueError, match='records'):
        stage.apply({k: torch.from_numpy(v[:1]) for k, v in rec.items()})
    # the wrapper of a source of full batches: the first half and its reverses
    class Source:
        def next(self):
            return {k: torch.from_numpy(v) for k, v in P.mirror_host(rec).items()}
    out = P.PairSwappedData(Source(), stage).next()
    for k in rec:
        assert out[k].numpy().tobytes() == want[k].tobytes(), k


def test_key_handling():
    assert P.pair_swap_from_conf({}) is False and P.pair_swap_from_conf({'pair_swap': None}) is False
    assert P.pair_swap_from_conf({'pair_swap': False, 'batch_size': 3}) is False
    assert P.pair_swap_from_conf({'pair_swap': True, 'batch_size': 4}) is True
    for bad in (1, 0, 'yes', 1.0):
        with pytest.raises(ValueError, match='pair_swap'):
            P.pair_swap_from_conf({'pair_swap': bad, 'batch_size': 4})
    for odd in (3, 1, 0, None, 4.0):
        with pytest.raises(ValueError, match='batch_size'):
            P.pair_swap_from_conf({'pair_swap': True, 'batch_size': odd})
    with pytest.raises(ValueError, match='off'):
        P.PairSwap({'batch_size': 4})


def test_models_take_or_refuse_the_key():
    from dynamic_multiview_3d_amd import multiobject_main_model
    from dynamic_multiview_3d_amd.appearance_flow_model import AppearanceFlowModel
    from dynamic_multiview_3d_amd.multiobject_appflow import MultiObjectAppFlow
    base = {'learning_rate': 1e-4}
    with pytest.raises(ValueError, match='batch_size'):
        AppearanceFlowModel(dict(base, batch_size=3, pair_swap=True), load_tfrec=False, device='cpu')
    with pytest.raises(ValueError, match='pair_swap'):
        AppearanceFlowModel(dict(base, batch_size=2, pair_swap=1), load_tfrec=False, device='cpu')
    mo = dict(base, batch_size=2, use_color='', combination_image='', fully_conv='', pair_swap=True)
    for cls in (MultiObjectAppFlow, multiobject_main_model.Base_Prediction_Model):
        with pytest.raises(ValueError, match='pair_swap'):
            cls(mo, load_tfrec=False, device='cpu')
    m = AppearanceFlowModel(dict(base, batch_size=2, pair_swap=True), load_tfrec=False, device='cpu')
    assert set(m.graph.inputs) == set(P.NAMES)


def test_base_prediction_model_batches_go_through_the_stage_under_their_own_names():
    """Base_Prediction_Model names its depth inputs dimage0 / dimage1: the synthetic feed of train.py, mirrored, has the layout."""
    from dynamic_multiview_3d_amd.main_model import Base_Prediction_Model
    from dynamic_multiview_3d_amd.train import SyntheticData
    conf = {'batch_size': 4, 'learning_rate': 1e-4, 'use_color': '', 'use_depth': '', 'depth_lr_factor': 0.1, 'pair_swap': True}
    m = Base_Prediction_Model(conf, load_tfrec=False, device='cpu')
    assert set(m.graph.inputs) == {'image0', 'image1', 'dimage0', 'dimage1', 'disp'}
    assert P.swapped_pairs(m.graph.inputs) == (('image0', 'image1'), ('dimage0', 'dimage1'))
    source = SyntheticData(m, seed=2, pool=2)
    stage = P.PairSwap(conf, next(iter(m.graph.inputs.values())).shape[0])
    data = P.PairSwappedData(source, stage)
    for t in range(2):
        raw = {k: v.numpy().copy() for k, v in source.pool[t].items()}
        batch = {k: v.numpy() for k, v in data.next().items()}
        assert list(batch) == list(m.graph.inputs)
        for k, t_in in m.graph.inputs.items():
            assert batch[k].shape == tuple(t_in.shape) and batch[k][:2].tobytes() == raw[k][:2].tobytes(), k
        for x, y in (('image0', 'image1'), ('dimage0', 'dimage1')):
            assert batch[x][2:].tobytes() == raw[y][:2].tobytes() and batch[y][2:].tobytes() == raw[x][:2].tobytes(), x
        assert batch['disp'][2:].tobytes() == np.negative(raw['disp'][:2]).tobytes()
        m.feed(**batch)                                                   # the graph takes the names and the shapes
    want = P.mirror_host({k: v[:2] for k, v in raw.items()})
    assert all(want[k].tobytes() == batch[k].tobytes() for k in raw)
    with pytest.raises(ValueError, match='exactly the inputs'):           # both depth pairs at once are no model's inputs
        P.swapped_pairs(list(P.NAMES) + ['dimage0', 'dimage1'])


def test_the_stage_takes_the_graphs_batch_per_rank_and_per_micro_batch(tmp_path):
    """conf['batch_size'] is the graph's batch: what one rank feeds per (micro-)step.  The stage is sized by the graph's batch where
    the caller knows it, and every batch a rank's reader hands out is mirrored on its own."""
    conf = {'batch_size': 4, 'pair_swap': True, 'grad_accum_steps': 2}
    assert P.PairSwap(conf).half == 2 and P.PairSwap(conf, 6).half == 3
    with pytest.raises(ValueError, match='even batch'):
        P.PairSwap(conf, 5)
    _write_shards(tmp_path, nfiles=4)
    rconf = dict(conf, data_dir=str(tmp_path), train_val_split=1.0, test_mode='')
    seen = []
    for rank in (0, 1):
        for batch in _take(R.TFRecordInput(rconf, SHAPES, device='cpu', rank=rank, world=2), 3):      # three micro-batches per rank
            _check_layout(batch, B // 2)
            seen.append(batch['disp'][:B // 2].tobytes())
    assert len(set(seen)) == len(seen)                                    # the ranks read different shards


# ------------------------------------------------------------------------------------------------ the reader
def _write_shards(tmp_path, nfiles=3, per_file=3, seed=0):
    rng = np.random.default_rng(seed)
    recs = []
    for f in range(nfiles):
        with R.TFRecordWriter(str(tmp_path / ('%d.tfrecords' % f))) as w:
            for _ in range(per_file):
                r = {'image0': rng.integers(0, 256, (H, H, 3), dtype=np.uint8), 'image1': rng.integers(0, 256, (H, H, 3), dtype=np.uint8),
                     'depth0': rng.integers(0, 256, (H, H, 1), dtype=np.uint8), 'depth1': rng.integers(0, 256, (H, H, 1), dtype=np.uint8),
                     'displacement': rng.uniform(-1, 1, 2).astype(np.float32)}
                recs.append(r)
                w.write(R.serialize_example({k: (v.tobytes() if v.dtype == np.uint8 else v) for k, v in r.items()}))
    return recs


def _take(inp, count):
    try:
        return [{k: v.numpy().copy() for k, v in inp.next().items()} for _ in range(count)]
    finally:
        inp.close()


def test_the_reader_consumes_half_as_many_records_in_the_same_order(tmp_path):
    recs = _write_shards(tmp_path)                                        # 9 records: batches straddle files and the epoch
    conf = {'batch_size': B, 'data_dir': str(tmp_path), 'train_val_split': 1.0, 'test_mode': ''}
    off = _take(R.TFRecordInput(conf, SHAPES, device='cpu'), 5)
    assert off == [] or all(v.shape[0] == B for v in off[0].values())
    flat = {k: np.concatenate([b[k] for b in off]) for k in SHAPES}      # the key-off order, 20 records
    for i in range(20):                                                   # ... which is the file order, wrapping after 9
        assert flat['image0'][i].tobytes() == (recs[i % 9]['image0'].astype(np.float32) / np.float32(255)).tobytes()
    for value in (None, False):                                           # off: the same batches, bit for bit
        same = _take(R.TFRecordInput(dict(conf, pair_swap=value), SHAPES, device='cpu'), 5)
        assert all(a[k].tobytes() == b[k].tobytes() for a, b in zip(off, same) for k in SHAPES)
    for training in (True, False):                                        # the layout belongs to the batch, not to training
        on = _take(R.TFRecordInput(dict(conf, pair_swap=True), SHAPES, training=training, device='cpu'), 8)
        for t, batch in enumerate(on):
            assert all(batch[k].shape == SHAPES[k] and batch[k].dtype == np.float32 for k in SHAPES)
            for k in SHAPES:                                              # batch t holds records t B/2 .. (t+1) B/2 - 1
                assert batch[k][:B // 2].tobytes() == flat[k][t * (B // 2):(t + 1) * (B // 2)].tobytes(), (t, k)
            _check_layout(batch, B // 2)


def test_the_mirror_runs_behind_the_colour_augmentation(tmp_path):
    _write_shards(tmp_path)
    conf = dict({'batch_size': B, 'data_dir': str(tmp_path), 'train_val_split': 1.0}, **CC.CONF)
    plain = _take(R.TFRecordInput({k: v for k, v in conf.items() if not k.startswith('augment')}, SHAPES, device='cpu', seed=3), 6)
    flat = {k: np.concatenate([b[k] for b in plain]) for k in SHAPES}    # the (shuffled, seeded) key-off order without augmentation
    on = _take(R.TFRecordInput(dict(conf, pair_swap=True), SHAPES, device='cpu', seed=3), 6)
    changed = 0
    for t, batch in enumerate(on):
        _check_layout(batch, B // 2)                                      # image0[n + B/2] == image1[n] bit for bit, after augmentation
        lo, hi = t * (B // 2), (t + 1) * (B // 2)
        for k in ('depth_image0', 'depth_image1', 'disp'):                # what the colour stage leaves alone names the records
            assert batch[k][:B // 2].tobytes() == flat[k][lo:hi].tobytes(), (t, k)
        changed += int(batch['image0'][:B // 2].tobytes() != flat['image0'][lo:hi].tobytes())
        assert batch['image0'].min() >= 0.0 and batch['image0'].max() <= 1.0
    assert changed == len(on)                                             # the colour stage did run on every batch
    # validation inputs are never augmented, and are mirrored all the same
    val = _take(R.TFRecordInput(dict(conf, pair_swap=True, train_val_split=0.0), SHAPES, training=False, device='cpu', seed=3), 2)
    for batch in val:
        _check_layout(batch, B // 2)


def test_the_reader_refuses_an_odd_batch_and_a_non_bool(tmp_path):
    _write_shards(tmp_path, nfiles=1)
    conf = {'batch_size': 3, 'data_dir': str(tmp_path), 'train_val_split': 1.0, 'test_mode': '', 'pair_swap': True}
    odd = {k: (3,) + s[1:] for k, s in SHAPES.items()}
    with pytest.raises(ValueError, match='batch_size'):
        R.TFRecordInput(conf, odd, device='cpu')
    with pytest.raises(ValueError, match='pair_swap'):
        R.TFRecordInput(dict(conf, batch_size=4, pair_swap='on'), SHAPES, device='cpu')
