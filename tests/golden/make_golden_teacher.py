"""Generate tests/golden/teacher.npz and tests/golden/signatures_teacher.json by running the REFERENCE (mesnico/ALADIN) teacher:
`get_teacher_scores`, alad/train.py:340-384, over the reference's own ImageBertForSequenceClassification
(oscar/modeling/modeling_bert.py:290-350) with `output_attentions=True`, eval mode, float64.

Like make_golden.py: gen_backbone (whose conventions it follows) the reference's model runs over tests/golden/hf_bert_layers.py standing
in for the un-vendored `transformers.pytorch_transformers` layers.  Runs ONLY where the reference is importable and copies none of it.

Route 'reference_function': alad.train is imported with every module that is not installed where the generator runs (tqdm,
tensorboard, the tokenizer of the un-vendored transformers, ...) replaced by an empty stand-in, and ITS get_teacher_scores is called.  Route 'recorded_outputs' (taken if that import fails): the reference model's
logits and attentions[-1] are recorded per chunk and teacher_numpy.teacher_bookkeeping restates the five lines after the model
call.  The route taken is stored in the file.

    per case    the generator arguments (JSON), input checksums, scores (Bi, Bc), attentions (Bi, Bc, 69, 12) (float64)

    python tests/golden/make_golden_teacher.py
"""
import importlib
import importlib.util
import json
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'helpers'))

import numpy as np
import torch

import make_golden as MG                          # noqa: E402  (reference on the path: t, signature_record)
import teacher_numpy as TN                        # noqa: E402
from aladin_amd import synth                      # noqa: E402

NAME = 'teacher'


class _Stub(types.ModuleType):
    """a module that is not installed: any attribute is a fresh stand-in class, any submodule another stub"""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return type(name, (), {})


def reference_modules():
    """-> (the reference's modeling_bert over hf_bert_layers, alad.train or None)"""
    spec = importlib.util.spec_from_file_location('transformers.pytorch_transformers.modeling_bert', os.path.join(HERE, 'hf_bert_layers.py'))
    layers = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(layers)
    import transformers                            # noqa: F401  (the installed one: its name space takes the stand-in submodule)
    pkg = _Stub('transformers.pytorch_transformers')
    pkg.modeling_bert = layers
    pkg.BertConfig = layers.BertConfig
    mu = types.ModuleType('oscar.modeling.modeling_utils')
    mu.CaptionPreTrainedModel = type('CaptionPreTrainedModel', (layers.BertPreTrainedModel,), {})
    mu.ImgPreTrainedModel = type('ImgPreTrainedModel', (layers.BertPreTrainedModel,), {})
    cbs = types.ModuleType('oscar.utils.cbs')
    cbs.ConstrainedBeamSearch = cbs.select_best_beam_with_constraints = None
    sys.modules.update({'transformers.pytorch_transformers': pkg, 'transformers.pytorch_transformers.modeling_bert': layers,
                        'oscar.modeling.modeling_utils': mu, 'oscar.utils.cbs': cbs})
    sys.modules.pop('oscar.modeling.modeling_bert', None)
    ref_mb = importlib.import_module('oscar.modeling.modeling_bert')
    assert ref_mb.__file__.startswith('/root/reference/')
    train = None
    try:
        importlib.import_module('torch.utils.tensorboard')
    except ImportError:                            # present in torch, but refuses to load without the tensorboard package
        sys.modules['torch.utils.tensorboard'] = _Stub('torch.utils.tensorboard')
    for _ in range(64):                            # one stand-in per missing module, then try again
        try:
            train = importlib.import_module('alad.train')
            break
        except ModuleNotFoundError as e:
            if not e.name or e.name.startswith('alad.train'):
                break
            parts = e.name.split('.')
            for i in range(1, len(parts) + 1):
                sys.modules.setdefault('.'.join(parts[:i]), _Stub('.'.join(parts[:i])))
        except Exception as e:                     # noqa: BLE001
            print('alad.train is not importable here: %r' % (e,))
            break
    if train is not None:
        assert train.__file__.startswith('/root/reference/')
    return layers, ref_mb, train


def main():
    layers, ref_mb, train = reference_modules()
    route = 'reference_function' if train is not None else 'recorded_outputs'
    rec = {'n_cases': np.int64(len(TN.GOLDEN_CASES)), 'route': np.array(route), 'text_len': np.int64(TN.TEXT_LEN)}
    for ci, (name, n, num_labels, subdivs, seed) in enumerate(TN.GOLDEN_CASES):
        cfg_kw = TN.golden_cfg(num_labels)
        cfg = layers.BertConfig(output_attentions=True, output_hidden_states=False, **cfg_kw)
        torch.manual_seed(0)
        ref = ref_mb.ImageBertForSequenceClassification(cfg).eval().double()
        named = [(k, tuple(p.shape)) for k, p in ref.named_parameters()]
        vals = synth.module_parameters(named, TN.PARAM_SEED, scale=TN.PARAM_SCALE)
        with torch.no_grad():
            for k, p in ref.named_parameters():
                p.copy_(MG.t(vals[k]).double())
        ids, mask, types_, feats, labels = TN.golden_inputs(n, seed)
        batch = (MG.t(ids), MG.t(mask), MG.t(types_), MG.t(feats).double(), MG.t(labels))
        side = int(round(n ** 0.5))
        if train is not None:
            args = types.SimpleNamespace(device=torch.device('cpu'), num_labels=num_labels)
            scores, att = train.get_teacher_scores(args, ref, batch, subdivs)
            scores, att = scores.numpy(), att.numpy()
        else:
            logits, wins = [], []
            with torch.no_grad():
                for b in range(0, n, subdivs):
                    e = b + subdivs
                    o = ref(input_ids=batch[0][b:e], attention_mask=batch[1][b:e], token_type_ids=batch[2][b:e], img_feats=batch[3][b:e])
                    logits.append(o[0].numpy())
                    wins.append(o[1][-1].numpy().mean(axis=1)[:, 1:TN.TEXT_LEN, TN.TEXT_LEN:])
            scores, att = TN.teacher_bookkeeping(np.concatenate(logits), np.concatenate(wins), num_labels, (side, side))
        assert scores.shape == (side, side) and att.shape == (side, side, TN.TEXT_LEN - 1, TN.N_REGIONS), (scores.shape, att.shape)
        assert scores.dtype == np.float64 and att.dtype == np.float64
        pre = 'c%d_' % ci
        rec[pre + 'name'] = np.array(name)
        rec[pre + 'args'] = np.array(json.dumps(dict(n=n, num_labels=num_labels, subdivs=subdivs, seed=seed, cfg=cfg_kw,
                                                       param_seed=TN.PARAM_SEED, param_scale=TN.PARAM_SCALE), sort_keys=True))
        rec[pre + 'param_names'] = np.array([k for k, _ in named])
        rec[pre + 'ids_checksum'] = np.float64(synth.checksum(ids))
        rec[pre + 'mask_checksum'] = np.float64(synth.checksum(mask))
        rec[pre + 'feats_checksum'] = np.float64(synth.checksum(feats))
        rec[pre + 'scores'] = scores
        rec[pre + 'attentions'] = att
        print('%-20s route %s  scores %s in [%.4g, %.4g]  attentions %s max %.4g  masked-region mass %.3g'
              % (name, route, scores.shape, scores.min(), scores.max(), att.shape, att.max(),
                 float((att * (1 - mask[:, TN.TEXT_LEN:]).reshape(side, side, 1, -1)).max())))
    path = os.path.join(HERE, NAME + '.npz')
    np.savez_compressed(path, **rec)
    print('%s: %d bytes' % (path, os.path.getsize(path)))
    sig = {}
    if train is not None:
        sig['get_teacher_scores'] = MG.signature_record(train.get_teacher_scores)
    sig['ImageBertForSequenceClassification.forward'] = MG.signature_record(ref_mb.ImageBertForSequenceClassification.forward)
    with open(os.path.join(HERE, 'signatures_%s.json' % NAME), 'w') as f:
        json.dump(sig, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()
