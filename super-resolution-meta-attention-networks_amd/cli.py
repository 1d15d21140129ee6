"""train_sisr / eval_sisr entry points (same TOML schema and outputs as the reference's console scripts).

ref: Code/SISR/net_train.py:16-74 (experiment_setup), Code/SISR/training/training_handler.py:25-323
     (TrainingHandler: epoch loop, Y-PSNR / Y-SSIM validation, summary.csv, per-epoch checkpoints, early stopping),
     Code/SISR/net_eval.py:20-74 + Code/SISR/evaluation/standard_eval.py:217-319 (full_image_protocol).
Run:  python -m sisr_cli train --parameters cfg.toml      |      python -m sisr_cli eval --config cfg.toml
With WORLD_SIZE > 1 (torch.distributed.run) training is data parallel: every rank walks the same seeded
loader and takes its contiguous shard of each batch; rank 0 validates, logs and checkpoints.
"""
import argparse
import math
import os
import random
import time
from collections import defaultdict

import numpy as np
import torch

from . import metrics as M
from . import parallel
from .data import SuperResImages, rgb_to_ycbcr, sisr_data_setup
from .handlers import ModelInterface, QModel, create_dir_if_empty


def _load_toml(path):
    import tomli
    with open(path, 'rb') as f:
        return tomli.load(f)


def _dump_toml(d, path):
    def fmt(v):
        if isinstance(v, bool):
            return 'true' if v else 'false'
        if isinstance(v, (int, float)):
            return repr(v)
        if isinstance(v, (list, tuple)):
            return '[' + ', '.join(fmt(x) for x in v) + ']'
        return '"' + str(v).replace('\\', '\\\\').replace('"', '\\"') + '"'

    lines = []

    def emit(table, prefix):
        for k, v in table.items():
            if not isinstance(v, dict) and v is not None:
                lines.append(f'{k} = {fmt(v)}')
        for k, v in table.items():
            if isinstance(v, dict):
                lines.append(f'\n[{prefix + k}]')
                emit(v, prefix + k + '.')
    emit(d, '')
    with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')


class TrainingHandler:
    def __init__(self, experiment_name, save_loc, model_params, data_params, gpu='off', sp_gpu=0, num_epochs=None,
                 continue_from_epoch=None, max_im_val=1.0, metrics=None, seed=8, epoch_cutoff=None,
                 early_stopping_patience=None, overwrite_data=False, device_metrics=False, psnr_shave=None, **kwargs):
        """device_metrics: validation through ModelInterface.net_run_and_measure -- the output stays on the model's device, PSNR
        comes from the device output stage (metrics.eval_output) and only the per-image values cross to the host; on a CPU
        model the host forms of the same functions.  psnr_shave: pixels cropped from every border before PSNR (the papers'
        protocol, typically the scale); needs device_metrics."""
        self.device_metrics = bool(device_metrics)
        if psnr_shave is not None and not self.device_metrics:
            raise ValueError("[training] psnr_shave is honoured by the device output stage only: set device_metrics = true with it")
        self.psnr_shave = int(psnr_shave or 0)
        self.rank, self.world, local = parallel.init_distributed()
        self.num_epochs, self.stop_patience, self.overwrite = num_epochs, early_stopping_patience, bool(overwrite_data)
        torch.manual_seed(seed)
        torch.cuda.manual_seed_all(seed)
        np.random.seed(seed)
        random.seed(seed)
        self.best_val_model_idx, self.best_val_model_psnr = 0, 0
        self.best_val_model_loss = None  # (models that predict the degradation code are ranked by val-loss)
        self.max_im_val = max_im_val
        self.metrics = list(metrics) if metrics is not None else None
        if self.world > 1:
            if os.environ.get("SISR_BENCH_SHARE_GPU"):  # rehearsal on a 1-GPU box: every rank on cuda:0
                local = 0
            gpu, sp_gpu = 'multi', local
        if self.rank != 0 and os.path.isdir(save_loc):
            pass  # every rank builds the interface; only rank 0 writes checkpoints / logs
        self.model = ModelInterface(save_loc, experiment_name, gpu=gpu, sp_gpu=int(sp_gpu), mode='train',
                                    new_params=model_params, load_epoch=continue_from_epoch)
        self.starting_epoch = self.model.model_epoch
        if self.starting_epoch > 0:
            self.starting_epoch += 1
        if epoch_cutoff is not None:
            self.num_epochs = epoch_cutoff - self.starting_epoch
        self.train_data, self.val_data = sisr_data_setup(scale=model_params['internal_params']['scale'],
                                                         device=self.model.model.device,
                                                         **self.model.configuration, **data_params)

    def train(self):
        losses = defaultdict(list)
        for batch in self.train_data:
            n = len(batch['tag'])
            if self.world > 1:
                batch = parallel.shard_batch(batch, self.rank, self.world)
            loss, _ = self.model.train_batch(**batch)
            if self.world > 1:  # logging only: the mean over the global batch from the ranks' shard means
                mine = len(batch['tag'])
                t = torch.tensor([float(loss) * mine if mine else 0.0, float(mine)], dtype=torch.float64)
                if torch.distributed.get_backend() == 'nccl':
                    t = t.to(self.model.model.device)
                torch.distributed.all_reduce(t)
                loss = np.float32(t[0].item() / n)
            losses['train-loss'].append(loss)
        losses['learning-rate'].append(self.model.get_learning_rate())
        self.model.epoch_end_calls()
        return losses

    def eval(self, epoch_idx):
        """validation on the averaged weights when the model keeps an average (ema_decay): the best epoch is then chosen on
        what 'network_ema' of its checkpoint holds"""
        handler = self.model.model
        if getattr(handler, 'has_ema', None) is not None and handler.has_ema():
            with handler.averaged_weights():
                return self._eval(epoch_idx)
        return self._eval(epoch_idx)

    def _eval_codes(self):
        """validation of a model that predicts the degradation code (handler.predicts_metadata): per batch the loss against
        the batch's code and per image the mean absolute code error; no image is made, the `metrics` list is not read"""
        handler = self.model.model
        losses = defaultdict(list)
        for batch in self.val_data:
            codes, loss, _ = handler.run_eval(batch['lr'], metadata=batch['metadata'], metadata_keys=batch['metadata_keys'],
                                              request_loss=True)
            target = handler.target_codes(batch['lr'], batch['metadata'], batch['metadata_keys']).cpu()
            losses['val-loss'].append(loss)
            losses['val-MAE'].extend((codes.double() - target.double()).abs().mean(dim=1).tolist())
        return losses

    def _eval(self, epoch_idx):
        if getattr(self.model.model, 'predicts_metadata', False):
            return self._eval_codes()
        losses = defaultdict(list)
        wanted = list(dict.fromkeys(self.metrics or ()))  # columns follow the order the metrics are listed in
        for batch in self.val_data:
            y = batch['hr']
            if self.device_metrics:
                measured, loss, _, _ = self.model.net_run_and_measure(**batch, metrics=wanted, max_value=self.max_im_val,
                                                                      shave=self.psnr_shave, request_loss=True)
                losses['val-loss'].append(loss)
                for metric in wanted:
                    if metric in measured:
                        losses['val-' + metric].extend(measured[metric])
                continue
            if 'SSIM' in wanted or 'MS-SSIM' in wanted:  # measured on the device output, before it is copied back
                rgb_out, ycbcr_out, loss, _, measured = self.model.net_run_process_and_measure(
                    **batch, metrics=wanted, max_value=self.max_im_val, request_loss=True)
            else:
                rgb_out, ycbcr_out, loss, _ = self.model.net_run_and_process(**batch, request_loss=True)
                measured = {}
            if 'rgb' in self.model.configuration['colorspace']:
                y_proc = self.model.colorspace_convert(y, colorspace='rgb')
            else:  # ref training_handler.py:194-197: a Y-channel model's reference images already are YCbCr
                y_proc = self.model._standard_image_formatting(y.numpy())
            losses['val-loss'].append(loss)
            for metric in wanted:
                if metric == 'PSNR':
                    for i in range(ycbcr_out.shape[0]):
                        losses['val-PSNR'].append(M.psnr(ycbcr_out[i, 0], y_proc[i, 0], max_value=self.max_im_val))
                elif metric == 'SSIM':
                    losses['val-SSIM'].extend(measured['SSIM'])
                elif metric == 'MS-SSIM':
                    losses['val-MS-SSIM'].extend(measured['MS-SSIM'])
        return losses

    def run_experiment(self):
        import pandas as pd
        total = defaultdict(list)
        summary = os.path.join(self.model.logs, 'summary.csv')
        if self.starting_epoch != 0 and os.path.isfile(summary):
            old = pd.read_csv(summary)
            total = defaultdict(list, {k: list(old[k]) for k in old.columns})
        stale = 0
        for i, epoch_idx in enumerate(range(self.starting_epoch, self.starting_epoch + self.num_epochs)):
            t0 = time.time()
            print('Running epoch', epoch_idx)
            self.model.set_epoch(epoch_idx)
            if i == 0 and self.rank == 0:
                self.model.save(override=self.overwrite, dry_run=True)
            cur = dict(self.train())
            if self.rank != 0:
                iter(self.val_data)  # rank 0's validation iterator draws its base seed from the global torch RNG: keep
                #                      every rank's stream -- hence next epoch's shuffle -- identical
            if self.rank == 0:
                cur.update(self.eval(epoch_idx))
                if getattr(self.model.model, 'predicts_metadata', False):  # no image, no PSNR: the lowest val-loss is best
                    val_loss = float(np.mean(cur['val-loss']))
                    improved = self.best_val_model_loss is None or val_loss < self.best_val_model_loss
                    if improved:
                        self.best_val_model_loss = val_loss
                else:
                    val_psnr = np.mean(cur['val-PSNR']) if 'val-PSNR' in cur else float('nan')
                    improved = val_psnr > self.best_val_model_psnr
                    if improved:
                        self.best_val_model_psnr = val_psnr
                if improved:
                    self.best_val_model_idx, stale = epoch_idx, 0
                else:
                    stale += 1
                for k, v in cur.items():
                    avg = np.nanmean(v)
                    total[k].append(0 if math.isnan(avg) else avg)
                total['epoch'].append(epoch_idx)
                self.model.save(override=self.overwrite)
                pd.DataFrame(total).to_csv(summary, index=False)
                print("Epoch {}:".format(epoch_idx), " ".join("{}_{:.4f}".format(k, np.mean(v)) for k, v in cur.items()),
                      "Epoch duration: {:.4f} seconds".format(time.time() - t0))
            if self.world > 1:
                flag = torch.tensor([1.0 if stale == self.stop_patience else 0.0], device=self.model.model.device)
                torch.distributed.broadcast(flag, src=0)
                if flag.item():
                    break
            elif self.stop_patience is not None and stale == self.stop_patience:
                print('Stopping model training, validation loss has plateaued.')
                break
        return total


def train_sisr(parameters, experiment_name=None, **overrides):
    """ref: net_train.py:29-74.  `parameters`: TOML path or an already-loaded dict."""
    params = _load_toml(parameters) if isinstance(parameters, str) else parameters
    params.setdefault('training', {}).update({k: v for k, v in overrides.items() if v is not None})
    if experiment_name is not None:
        params['experiment'] = experiment_name
    model = params['model']
    ml = model['internal_params'].get('metadata_list')
    if ml is not None:
        with open(ml) as f:
            model['internal_params']['metadata'] = [line.rstrip() for line in f]
    exp = TrainingHandler(experiment_name=params['experiment'], save_loc=params['experiment_save_loc'],
                          model_params=model, data_params=dict(params['data']), **params['training'])
    if exp.rank == 0:
        cont = params['training'].get('continue_from_epoch')
        _dump_toml(params, os.path.join(exp.model.base_folder,
                                        'config.toml' if cont is None else 'config_from_epoch_%s.toml' % cont))
        exp.model.save_metadata()
    return exp.run_experiment()


def _low_res_prep(lr, scale):
    """ref: standard_eval.py:146-158: each image of a (B, 3, h, w) fp32 host batch through ToPILImage (`mul(255).byte()`), PIL's
    `resize((w * scale, h * scale), BICUBIC)` and ToTensor -> (B, 3, h * scale, w * scale) fp32.  The host form of
    degrade.pil_bicubic_upsample: used when the models run on the CPU, and what the device kernel is tested against."""
    from PIL import Image
    from .data import to_tensor
    out = torch.empty(*lr.shape[0:2], lr.shape[2] * scale, lr.shape[3] * scale)
    for i in range(lr.shape[0]):
        image = Image.fromarray(lr[i].mul(255).byte().permute(1, 2, 0).contiguous().numpy())
        out[i] = to_tensor(image.resize((image.width * scale, image.height * scale), resample=Image.BICUBIC))
    return out


def _interpolated(lr, scale, device, want_ycbcr, timing):
    """The interpolated RGB batch, its YCbCr form (or None) and the seconds it took (or None): on `device` from the uploaded LR
    batch (one launch for both), or on the host (ref: standard_eval.py:236-241)."""
    tic = None
    if device is not None:
        from . import degrade
        lr = lr.to(device)
        if timing:
            torch.cuda.synchronize(device)
            tic = time.perf_counter()
        out = degrade.pil_bicubic_upsample(lr, scale, rgb=True, ycbcr=want_ycbcr)
        rgb, ycbcr = out if want_ycbcr else (out, None)
        if timing:
            torch.cuda.synchronize(device)
    else:
        if timing:
            tic = time.perf_counter()
        rgb = _low_res_prep(lr, scale)
        ycbcr = torch.from_numpy(M.batch_rgb_to_ycbcr(rgb.numpy())) if want_ycbcr else None
    return rgb, ycbcr, time.perf_counter() - tic if timing else None


def _load_predictor(cfg, models):
    """The `metadata_predictor = [experiment, epoch]` model of an evaluation (None without the key), loaded once next to the
    listed models.  Every listed Q-model must take exactly the code it predicts: a different `metadata` list, in order or
    content, is refused here, before any image is read."""
    key = cfg.get('metadata_predictor')
    if not key:
        return None
    name, ep = key
    use_ema = bool(cfg.get('use_ema'))
    if use_ema:  # the averaged weights when the predictor's run kept an average; its trained ones otherwise
        stored = _load_toml(os.path.join(cfg['model_loc'], name, 'config.toml'))['model']['internal_params']
        use_ema = stored.get('ema_decay') is not None
    predictor = ModelInterface(cfg['model_loc'], name, gpu='single' if cfg.get('gpu') else 'off', sp_gpu=cfg.get('sp_gpu', 0),
                               mode='eval', load_epoch=ep if ep in ('best', 'last') else int(ep), ema=use_ema)
    if not getattr(predictor.model, 'predicts_metadata', False):
        raise ValueError("metadata_predictor: experiment %r holds a %r model, which predicts no degradation code"
                         % (name, predictor.name))
    for m in models:
        if isinstance(m.model, QModel) and list(m.model.metadata) != list(predictor.model.metadata):
            raise ValueError("metadata_predictor: model %r reads the metadata %s, the predictor %r estimates %s; the two lists "
                             "must be the same, in the same order"
                             % (m.experiment, list(m.model.metadata), name, list(predictor.model.metadata)))
    return predictor


def _load_corrector(cfg, predictor):
    """The `ikc = { corrector = [experiment, epoch], iterations = 7 }` model of an evaluation -> (model | None, iterations).
    It corrects the code of `metadata_predictor`, which is required with it and must estimate the same `metadata` list (so
    every listed Q-model, checked against the predictor, takes the corrected code as well)."""
    key = cfg.get('ikc')
    if not key:
        return None, 0
    if predictor is None:
        raise ValueError("ikc: the loop corrects the code of metadata_predictor; set metadata_predictor = [experiment, epoch] "
                         "with it")
    name, ep = key['corrector']
    iterations = int(key.get('iterations', 7))
    if iterations < 1:
        raise ValueError("ikc: iterations must be at least 1 (got %r)" % (iterations,))
    use_ema = bool(cfg.get('use_ema'))
    if use_ema:  # the averaged weights when the corrector's run kept an average; its trained ones otherwise
        stored = _load_toml(os.path.join(cfg['model_loc'], name, 'config.toml'))['model']['internal_params']
        use_ema = stored.get('ema_decay') is not None
    corrector = ModelInterface(cfg['model_loc'], name, gpu='single' if cfg.get('gpu') else 'off', sp_gpu=cfg.get('sp_gpu', 0),
                               mode='eval', load_epoch=ep if ep in ('best', 'last') else int(ep), ema=use_ema)
    if not hasattr(corrector.model, 'correct'):
        raise ValueError("ikc: experiment %r holds a %r model, which corrects no degradation code" % (name, corrector.name))
    if list(corrector.model.metadata) != list(predictor.model.metadata):
        raise ValueError("ikc: the corrector %r corrects the metadata %s, the predictor %r estimates %s; the two lists must be "
                         "the same, in the same order" % (name, list(corrector.model.metadata), predictor.experiment,
                                                          list(predictor.model.metadata)))
    return corrector, iterations


def _code_columns(handler):
    """one column name per entry of a handler's code: the key itself, or key_<i> for a key of several entries"""
    names = []
    for key in handler.metadata:
        width = {'all': 40, 'blur_kernel': 10, 'unmodified_blur_kernel': 441}.get(key, 1)
        names += [key] if width == 1 else ['%s_%d' % (key, i) for i in range(width)]
    return names


def _code_rows(handler, batch, codes, have_file, iteration=None):
    """rows of predicted_metadata.csv for a batch: the code entries and, next to a metadata file, the mean absolute
    difference from the file's code; iteration (under `ikc`): the loop iteration the codes belong to, 0 = the predictor's"""
    host = codes.detach().cpu()
    names = _code_columns(handler)
    mae = None
    if have_file:
        want = handler.generate_channels(batch['lr'], batch['metadata'], batch['metadata_keys'])[:, :, 0, 0]
        mae = (host.double() - want.double()).abs().mean(dim=1).tolist()
    rows = []
    for i, tag in enumerate(batch['tag']):
        row = {'Image_Name': tag, **({} if iteration is None else {'iteration': iteration}),
               **{n: float(v) for n, v in zip(names, host[i].tolist())}}
        if mae is not None:
            row['code_MAE'] = mae[i]
        rows.append(row)
    return rows


def _with_predicted_codes(handler, predictor, batch, codes):
    """The batch a Q-model is given when its code comes from the predictor: the file's metadata is taken out and the
    predicted code goes in as `extra_channels` (QModel.channels_from_codes), on the model's device.  Handlers that build their
    own metadata maps, in run_eval (SRMD) or in generate_channels (SFTMD), get the code as the batch's metadata instead, keyed
    entry by entry."""
    feed = {k: v for k, v in batch.items() if k not in ('metadata', 'metadata_keys')}
    if type(handler).run_eval is QModel.run_eval and type(handler).generate_channels is QModel.generate_channels:
        extra = handler.channels_from_codes(codes)
        feed['extra_channels'] = extra if handler.device == torch.device('cpu') else extra.to(handler.device)
        return feed
    B = codes.shape[0]
    keys = [k for key in predictor.metadata
            for k in [key] * {'all': 40, 'blur_kernel': 10, 'unmodified_blur_kernel': 441}.get(key, 1)]
    feed['metadata'], feed['metadata_keys'] = codes.detach().cpu(), [tuple(k for _ in range(B)) for k in keys]
    return feed


def eval_sisr(config=None, **kw):
    """ref: net_eval.py:64-74 / standard_eval.py full_image_protocol: per-image and average Y-PSNR CSVs, plus Y-SSIM
    columns when the config's `metrics` lists 'SSIM' (ref: standard_eval.py:268-271) and Y-MS-SSIM columns when it lists
    'MS-SSIM' (metrics.batch_ms_ssim; no counterpart in the reference).  Each model is given the input its
    configuration names (ref: standard_eval.py:254-260): the LR batch as read, that batch bicubic-up-sampled x scale
    ('interp' models), or the up-sampled batch in YCbCr (the Y-channel models).  The up-sampled batch is made once per batch
    (on the device when the models run there), or read from `lr_dir_interp`.  `lr_baseline = true` adds 'LR' rows: the
    up-sampled image itself against the HR image (the reference always writes them).  `self_ensemble = true` evaluates
    `ikc = { corrector = ["<experiment>", <epoch>], iterations = 7 }` (with `metadata_predictor`) runs IKC's correction loop
    on the predictor's code (corrector.CorrectorHandler.correct) and gives every Q-model the final code; their rows carry
    '<experiment>~ikc' and predicted_metadata.csv one row per image and iteration.  `self_ensemble = true` evaluates
    every model with the geometric self-ensemble (run_eval(self_ensemble=True), the papers' "+" rows): its rows and its image
    folder carry the name '<experiment>+'; the LR rows are unaffected.  `use_ema = true` loads every listed model from the
    averaged weights of its checkpoint ('network_ema', stored by a run with ema_decay; a checkpoint without them is an
    error): its rows and image folder carry '<experiment>@ema' (before the '+', if both are set).  `device_outputs = true`
    routes every model through ModelInterface.net_run_and_measure: the HR batch is sent to the device once per batch for all
    models, PSNR and the listed metrics are measured on the device output, and with `save_im` the PNGs are written from the
    bytes the same launch makes (metrics.eval_output); no fp32 image crosses to the host.  Models on the CPU take the host
    forms of the same functions.  `psnr_shave = k` crops k pixels from every border before PSNR (the papers' protocol,
    typically k = scale; the model rows only); it needs device_outputs."""
    import pandas as pd
    cfg = dict(_load_toml(config)) if config is not None else {}
    cfg.update({k: v for k, v in kw.items() if v is not None})
    out_dir = os.path.join(cfg.get('out_loc', '.'), cfg.get('results_name', 'delete_me'))
    os.makedirs(out_dir, exist_ok=True)
    scale = cfg.get('scale', 4)
    models = [ModelInterface(cfg['model_loc'], name, gpu='single' if cfg.get('gpu') else 'off',
                             sp_gpu=cfg.get('sp_gpu', 0), mode='eval', load_epoch=ep if ep in ('best', 'last') else int(ep),
                             ema=bool(cfg.get('use_ema')))
              for name, ep in cfg['model_and_epoch']]
    for m in models:
        # A network fed the up-sampled image maps it to one of the same size whatever `scale` it was configured with (it
        # describes the crops of its training set: 1 where those were cut from interpolated images); the others must match.
        if m.configuration['input'] == 'unmodified' and scale != m.metadata['internal_params']['scale']:
            raise Exception('The model loaded has been trained for a different scale, '
                            'and cannot produce the requested images.')
    predictor = _load_predictor(cfg, models)
    corrector, ikc_iterations = _load_corrector(cfg, predictor)
    code_rows = []
    lr_dir = cfg['lr_dir']
    meta = cfg.get('metadata_file') or os.path.join(lr_dir, 'degradation_metadata.csv')
    if not os.path.isfile(meta):
        meta = None
    split = 'all' if cfg.get('full_directory') else (cfg.get('data_split') or 'eval')
    data = SuperResImages(lr_dir, cfg.get('hr_dir'), split=split,
                          dataset=cfg.get('dataset_name'), scale=scale, degradation_metadata_file=meta,
                          recursive_search=bool(cfg.get('recursive')))
    loader = torch.utils.data.DataLoader(dataset=data, batch_size=cfg.get('batch_size', 1))
    with_ssim = 'SSIM' in (cfg.get('metrics') or ())
    with_ms = 'MS-SSIM' in (cfg.get('metrics') or ())  # an 'MS-SSIM' column (five scales: images from 176 x 176)
    on_device = (['SSIM'] if with_ssim else []) + (['MS-SSIM'] if with_ms else [])
    timing = cfg.get('time_models', True)
    baseline = bool(cfg.get('lr_baseline'))
    plus = {'self_ensemble': True} if cfg.get('self_ensemble') else {}
    suffix = ('@ema' if cfg.get('use_ema') else '') + ('+' if plus else '')
    # rows and image folders of the Q-models that ran on the corrected code carry '<experiment>~ikc' (before '@ema' and '+')
    label = lambda m: m.experiment + ('~ikc' if corrector is not None and isinstance(m.model, QModel) else '') + suffix  # noqa: E731
    y_models = [m for m in models if 'rgb' not in m.configuration['colorspace']]
    need_interp = baseline or bool(y_models) or any(m.configuration['input'] != 'unmodified' for m in models)
    need_ycbcr = baseline or bool(y_models)
    device = next((torch.device('cuda', m.device) for m in models if m.device != torch.device('cpu')), None)
    device_outputs = bool(cfg.get('device_outputs'))
    if cfg.get('psnr_shave') is not None and not device_outputs:
        raise ValueError("psnr_shave is honoured by the device output stage only: set device_outputs = true with it")
    shave = int(cfg.get('psnr_shave') or 0)
    stored = None
    if need_interp and cfg.get('lr_dir_interp'):  # ready-made interpolated images, in step with the LR loader
        stored = iter(torch.utils.data.DataLoader(
            dataset=SuperResImages(cfg['lr_dir_interp'], cfg.get('hr_dir'), split=split, dataset=cfg.get('dataset_name'),
                                   scale=scale, input='interp', recursive_search=bool(cfg.get('recursive'))),
            batch_size=cfg.get('batch_size', 1)))
    rows = []
    for batch in loader:
        if baseline or not device_outputs:
            y_proc = ModelInterface.colorspace_convert(batch['hr'], colorspace='rgb')
        hr_there = hr_y_there = None  # the HR batch where the models run (RGB; YCbCr for the Y-channel models): sent once
        if device_outputs:
            hr_there = batch['hr'].to(device) if device is not None else batch['hr']
        interp = interp_ycbcr = None
        if stored is not None:
            interp, up_secs = next(stored)['lr'], None
            if need_ycbcr:
                interp_ycbcr = torch.from_numpy(M.batch_rgb_to_ycbcr(interp.numpy()))
        elif need_interp:
            interp, interp_ycbcr, up_secs = _interpolated(batch['lr'], scale, device, need_ycbcr, timing)
        if baseline:
            lr_y = interp_ycbcr[:, :1]
            if with_ssim:
                lr_ssim = M.batch_ssim(lr_y, torch.from_numpy(y_proc[:, :1]), max_value=1)
            if with_ms:
                lr_ms = M.batch_ms_ssim(lr_y, torch.from_numpy(y_proc[:, :1]), max_value=1)
            lr_y = lr_y.cpu().numpy()
            for i, tag in enumerate(batch['tag']):
                row = {'Image_Name': tag, 'Model': 'LR', 'PSNR': M.psnr(lr_y[i, 0], y_proc[i, 0], 1)}
                if with_ssim:
                    row['SSIM'] = lr_ssim[i]
                if with_ms:
                    row['MS-SSIM'] = lr_ms[i]
                row['runtime'] = up_secs
                rows.append(row)
        codes = None
        if predictor is not None:  # on the LR batch as read: RGB, before any interpolation
            codes, _, _ = predictor.model.run_eval(batch['lr'], keep_on_device=True)
            if corrector is None:
                code_rows.extend(_code_rows(predictor.model, batch, codes, have_file=meta is not None))
            else:  # IKC's loop on the image as read (the self-ensemble's eight variants all get the final code)
                _, codes, history = corrector.model.correct(batch['lr'], codes, ikc_iterations, want_sr=False)
                for iteration, h in enumerate(history):
                    code_rows.extend(_code_rows(predictor.model, batch, h, have_file=meta is not None, iteration=iteration))
        for m in models:
            feed = batch
            if codes is not None and isinstance(m.model, QModel):
                feed = _with_predicted_codes(m.model, predictor.model, batch, codes)
            if m in y_models:
                # the Y-channel branch reads the reference's Y from channel 0 of `hr` (loss, SSIM): hand it the HR image as
                # the validation set of such a model does, in YCbCr (data.SuperResImages, colorspace = 'ycbcr')
                feed = {**feed, 'lr': interp_ycbcr,
                        'hr': torch.stack([rgb_to_ycbcr(im, y_only=False) for im in batch['hr']])}
            elif m.configuration['input'] != 'unmodified':
                feed = {**feed, 'lr': interp}
            if device_outputs:
                if m in y_models:
                    if hr_y_there is None:
                        hr_y_there = feed['hr'].to(device) if device is not None else feed['hr']
                    feed = {**feed, 'hr': hr_y_there}
                else:
                    feed = {**feed, 'hr': hr_there}
                measured, _, secs, rgb8 = m.net_run_and_measure(**feed, metrics=['PSNR'] + on_device, max_value=1, shave=shave,
                                                                want_images=bool(cfg.get('save_im')), timing=timing, **plus)
                for i, tag in enumerate(batch['tag']):
                    row = {'Image_Name': tag, 'Model': label(m), 'PSNR': measured['PSNR'][i]}
                    for name in on_device:
                        row[name] = measured[name][i]
                    row['runtime'] = secs
                    rows.append(row)
                if cfg.get('save_im'):
                    from PIL import Image
                    d = os.path.join(out_dir, label(m))
                    os.makedirs(d, exist_ok=True)
                    for i, tag in enumerate(batch['tag']):
                        Image.fromarray(rgb8[i]).save(os.path.join(d, os.path.basename(tag)))
                continue
            if on_device:  # SSIM / MS-SSIM on the device output (data_range 1), outside the timed window
                rgb, ycbcr, _, secs, measured = m.net_run_process_and_measure(**feed, metrics=on_device, max_value=1,
                                                                              timing=timing, **plus)
            else:
                rgb, ycbcr, _, secs = m.net_run_and_process(**feed, timing=timing, **plus)
            for i, tag in enumerate(batch['tag']):
                row = {'Image_Name': tag, 'Model': label(m), 'PSNR': M.psnr(ycbcr[i, 0], y_proc[i, 0], 1)}
                if with_ssim:
                    row['SSIM'] = measured['SSIM'][i]
                if with_ms:
                    row['MS-SSIM'] = measured['MS-SSIM'][i]
                row['runtime'] = secs
                rows.append(row)
            if cfg.get('save_im'):
                from PIL import Image
                d = os.path.join(out_dir, label(m))
                os.makedirs(d, exist_ok=True)
                for i, tag in enumerate(batch['tag']):
                    Image.fromarray((rgb[i].transpose(1, 2, 0) * 255).round().astype(np.uint8)).save(
                        os.path.join(d, os.path.basename(tag)))
    df = pd.DataFrame(rows)
    mdir = os.path.join(out_dir, 'standard_metrics')
    create_dir_if_empty(mdir)
    df.to_csv(os.path.join(mdir, 'individual_metrics.csv'), index=False)
    if predictor is not None:
        pd.DataFrame(code_rows).to_csv(os.path.join(mdir, 'predicted_metadata.csv'), index=False)
    avg = df.groupby('Model')[['PSNR'] + on_device + ['runtime']].mean().reset_index()
    avg.to_csv(os.path.join(mdir, 'average_metrics.csv'), index=False)
    return df, avg


def main(argv=None):
    ap = argparse.ArgumentParser(prog='sisr_cli')
    sub = ap.add_subparsers(dest='cmd', required=True)
    t = sub.add_parser('train')
    t.add_argument('--parameters', required=True)
    t.add_argument('--num_epochs', type=int)
    t.add_argument('--gpu', choices=['single', 'multi'])
    t.add_argument('--sp_gpu')
    t.add_argument('--experiment_name')
    t.add_argument('--seed', type=int, default=8)
    t.add_argument('--continue_from_epoch', type=int)
    t.add_argument('--overwrite_data', action='store_true', default=None)
    e = sub.add_parser('eval')
    e.add_argument('--config', required=True)
    a = ap.parse_args(argv)
    if a.cmd == 'train':
        kw = {k: v for k, v in vars(a).items() if k not in ('cmd', 'parameters', 'experiment_name')}
        train_sisr(a.parameters, experiment_name=a.experiment_name, **kw)
    else:
        eval_sisr(a.config)
