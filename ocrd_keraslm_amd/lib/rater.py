"""Rater: character-level LSTM language model for rating text -- MI355X edition.

Drop-in for `ocrd_keraslm.lib.Rater` (ocrd_keraslm/lib/rating.py:12-1238): same
attributes, same methods, same status machine and assertion conventions.  The
seam the reference fills with a compiled Keras model (`self.model`,
rating.py:56) is filled here by `engine.HipLM`, which runs the network on
hand-written gfx950 kernels; everything in this file is host logic
(vocabulary, windowing, beam bookkeeping, training loop control).

Differences that are deliberate:
  * `streams` (new, default 1): number of independent stateful streams trained
    in lockstep per GPU.  1 reproduces the reference's batch_size=1 stateful
    training (rating.py:90-92); larger values are the data-parallel capability
    north_star asks for (each stream has its own carried state and reset points).
  * `segment_streams` (new, default False): with fewer training (or validation) files than streams, cut the
    files into contiguous segments on window boundaries and deal segments to the streams instead of files
    (segments.py); an epoch sees the same windows, the state is reset where a stream enters a segment.
  * `rate_batch` (new): `rate` for many independent texts at once, up to `streams`
    of them sharing each window call (ratebatch.py); every text is rated from a
    zero state, as `reset_states(1); rate(text)` would.
  * beam searches keep hypothesis states in a device-resident pool; `Node.state`
    is then a `StateRef`.  `predict()` called directly still takes and returns
    the reference's list-of-arrays states (rating.py:622-639).
  * context ids are clamped to the embedding range (the reference can index
    Embedding(200,10) out of range for years >= 1991, rating.py:111, 996).
  * the stateless, non-incremental window mode (rating.py:93-99, 352-378) runs through the
    same engine with `set_window_mode(True)`: zero state per window, one target per window.
"""
from __future__ import annotations

import json
import logging
import os
import signal
import time
from bisect import bisect_left, insort_left
from math import ceil, exp, log
from random import shuffle

import numpy as np

from . import genbeam, gensample, lattice_beam, modelio, ratebatch, ratebulk, segments, streams, windows
from .node import Node

PREC_BF16 = 1
PREC_SPLIT = 3


def _np(x):
    """engine results are torch tensors (HIP) or numpy arrays (test doubles)"""
    if hasattr(x, "detach"):
        return x.detach().cpu().numpy()
    return np.asarray(x)


def _target_probs(full, y):
    """the probability of the target y [B, T] in the distributions full [B, T, V]; 0.0 where there is no target (y < 0)"""
    p = np.take_along_axis(full, np.maximum(y, 0)[:, :, None], axis=2)[:, :, 0]
    return np.where(y >= 0, p, 0.0)


class StateRef(object):
    """Handle of one hypothesis state in the engine's device pool.  Quacks like
    the reference's state list [h1,c1,...,hL,cL] of (1,W) arrays when indexed."""
    __slots__ = ("pool", "slot", "head", "__weakref__")

    def __init__(self, pool, slot):
        self.pool = pool
        self.slot = slot
        self.head = None      # host copy of the first `depth` state vectors (what history clustering compares)

    def __del__(self):
        try:
            self.pool.release(self.slot)
        except Exception:
            pass

    def __len__(self):
        return 2 * self.pool.depth

    def __getitem__(self, k):
        return self.pool.fetch(self.slot)[k][None, :]

    def __bool__(self):
        return True


class StatePool(object):
    """Slot allocator over engine.pool ([slots][2L][W] f32 in HBM)."""

    def __init__(self, engine, depth, initial=1024):
        self.engine = engine
        self.depth = depth
        self.capacity = 0
        self.free = []
        self._grow(initial)
        self.zero_slot = self.take()      # never released: the all-zero state of `None`
        self.engine.pool_zero([self.zero_slot])

    def _grow(self, n):
        new = max(n, 2 * self.capacity)
        self.engine.ensure_pool(new)
        self.free.extend(range(new - 1, self.capacity - 1, -1))
        self.capacity = new

    def take(self):
        if not self.free:
            self._grow(2 * self.capacity)
        return self.free.pop()

    def release(self, slot):
        self.free.append(slot)

    def ref(self):
        return StateRef(self, self.take())

    @property
    def slot_bytes(self):
        """HBM one slot occupies (at the width the engine's kernels run at)"""
        return 2 * self.depth * int(getattr(self.engine, "pwidth", None) or self.engine.width) * 4

    def take_slots(self, n):
        """n bare slots for the duration of one engine call (the states in between of an edge walk); back with `release_slots`"""
        if n <= 0:
            return []
        while len(self.free) < n:
            self._grow(2 * self.capacity)
        slots = self.free[-n:]
        del self.free[-n:]
        slots.reverse()
        return slots

    def release_slots(self, slots):
        self.free.extend(reversed(slots))

    def refs(self, n):
        """n fresh handles at once (a beam search takes one per hypothesis and character)"""
        if n <= 0:                           # (free[-0:] is the whole list)
            return [], []
        while len(self.free) < n:
            self._grow(2 * self.capacity)
        slots = self.free[-n:]
        del self.free[-n:]
        slots.reverse()                      # (the order `take` would have handed them out in)
        return [StateRef(self, slot) for slot in slots], slots

    def fetch(self, slot):
        return self.engine.pool_read([slot])[0]


class Rater(object):
    '''A character-level RNN language model for rating text (see module docstring).

    Interfaces (as the reference, rating.py:25-32):
    - `Rater.train` : file handles of character sequences
    - `Rater.test` : file handles of character sequences
    - `Rater.rate2` (alias `rate_once`) : character string, one by one
    - `Rater.rate` : character string, all at once
    - `Rater.rate_best` : lattice graph
    - `Rater.rate_best_batch` : many independent lattice graphs at once
    - `Rater.generate` : alternative list of characters and states
    - `Rater.sample` : character strings drawn from the model's distribution
    '''

    def __init__(self, logger=None, engine_factory=None):
        # configuration variables (rating.py:39-47)
        self.width = 0
        self.depth = 0
        self.length = 0
        self.variable_length = True
        self.first_window = 0.1
        self.char_degradation = 0.01
        self.context_degradation = 0.1
        self.stateful = True
        self.mapping = ({}, {})
        # configuration constants (rating.py:49-51)
        self.batch_size = 128
        self.validation_split = 0.2
        self.smoothing = 0.2
        # runtime variables (rating.py:53-59)
        self.logger = logger or logging.getLogger(__name__)
        self.reset_cb = None
        self.incremental = False
        self.model = None
        self.history = {}
        self.status = 0
        self.voc_size = 0
        # MI355X additions
        self.streams = 1
        self.n_ctx = 1
        self.max_epochs = 100
        self.patience = 3
        self.seed = None
        self.device_dropout_masks = True     # ... and their dropout masks drawn on the device (False: by the host generator, as without batching)
        self.batched_streams = True          # the B streams of stateful training advanced together (streams.StreamBatcher)
        self.batched_streams_max_chars = 1 << 30
        self.edge_walk = False               # rate_best: every lattice edge's hypotheses walked through all their characters in ONE engine call (lattice_beam.walk_edge)
        self.edge_walk_slots = None          # ... slots one such call may be asked for (None: lattice_beam.walk_slot_budget of the pool's slot size)
        self.device_beam = os.environ.get('KERASLM_DEVICE_BEAM', '') == '1'      # generate: the beam's expansion and pruning on the device, the whole search enqueued without a wait (HipLM.beam_generate)
        self.sample_keep_probs = False      # sample: keep every step's probabilities in `sample_log` (tests look at what a pick saw)
        self.shared_left = None              # corrections(share_left=True): how many suspects and windows took which route, of the last call
        self.segment_streams = False         # fewer files than streams: cut the files into segments, one list of segments per stream (segments.py)
        self._engine_factory = engine_factory
        self._pool = None
        self._ctx_rows = None
        self._stop = False

    # ------------------------------------------------------------------ definition
    def configure(self):
        '''Define the model for the given parameters (rating.py:61-179).'''
        if self.stateful:
            self.variable_length = False
            self.first_window = 0
            self.batch_size = 1
        self.logger.info('using MI355X HIP implementation to compile %s %s model of depth %d width %d length %s size %d',
                         'stateful' if self.stateful else 'stateless',
                         'incremental' if self.incremental else 'contiguous',
                         self.depth, self.width,
                         'variable' if self.variable_length else str(self.length), self.voc_size)
        previous = self.model
        if self.voc_size > 0:
            factory = self._engine_factory
            if factory is None:
                from .engine import HipLM
                factory = HipLM
            self.model = factory(int(self.depth), int(self.width), int(self.voc_size), int(self.n_ctx))
            self.model.init_weights(seed=self.seed)
            # stateless contiguous graph (rating.py:98-99, 126-129): zero state per window, ONE output per window
            self.model.set_window_mode(not self.stateful and not self.incremental)
        else:
            self.model = None     # vocabulary unknown before the first training (rating.py:230)
        del previous
        self._pool = None
        self.status = 1

    def underspecify_contexts(self):
        '''Default input for context variables (rating.py:181-185).'''
        self.logger.info('using underspecification (zero) for %d context variables', self.n_ctx)
        return [0] * self.n_ctx

    # ------------------------------------------------------------------ training
    def train(self, data, val_data=None):
        '''Train model on text files (rating.py:248-310): stateful windows, one
        optimizer step per batch, validation after each epoch, early stopping with
        best-weights restore, per-epoch checkpoints, NaN abort, SIGINT graceful stop,
        state reset at file boundaries and before validation (callbacks.py:36-69).'''
        assert self.status > 0
        assert self.incremental is False
        if not self.stateful:
            return self._train_stateless(data, val_data)
        t_phase = time.perf_counter()
        self.timings = timings = {'split': 0.0, 'encode': 0.0, 'train_steps': 0.0, 'validation': 0.0, 'checkpoint': 0.0}
        (training_data, validation_data, _split, training_epoch_size, validation_epoch_size,
         total_size, steps) = self._split_data(data, val_data)
        timings['split'] = time.perf_counter() - t_phase
        self.logger.info('training on %d files / %d batches per epoch / %d character tokens for %d character types',
                         len(training_data), training_epoch_size, total_size, self.voc_size)
        self.reconfigure_for_mapping()
        lm = self.model
        if getattr(lm, "precision", PREC_BF16) != PREC_BF16:
            lm.prepare(PREC_BF16)
        sync = self._grad_sync()
        rank, world = sync.rank, sync.world
        sync.broadcast_params(lm)      # every rank initialised or loaded its own weights: rank 0's count
        B = max(1, int(self.streams))
        n_streams = B * world
        segment = bool(self.segment_streams)
        if not segment and (len(training_data) < n_streams or len(validation_data) < 1):
            assert n_streams == 1 or len(training_data) >= n_streams, \
                "need at least %d training files for %d streams (or segment_streams, which cuts the files into that many pieces)" \
                % (n_streams, n_streams)
        rng = np.random.default_rng(self.seed)
        reset_rows = set()

        def stream_items(files, train):
            """what is dealt to the streams: the files -- or, with `segment_streams` and fewer files than streams, their
            segments (file, lo, hi), the same plan on every rank (segments.plan).  Validation files with fewer windows than
            streams give one segment per window, and the streams left over fall back to the first item as they do with files."""
            if segment and len(files) < n_streams:
                cut = segments.char_plan([self._sizes[id(f)] for f in files], self.length, n_streams, strict=train)
                if cut:
                    return [(files[k], lo, hi) for k, lo, hi in cut]
            return list(files)

        training_items = stream_items(training_data, True)
        validation_items = stream_items(validation_data, False)
        if segment:
            self.logger.info('segment streams: %d training files in %d segments, %d validation files in %d segments, for %d streams',
                             len(training_data), len(training_items), len(validation_data), len(validation_items), n_streams)

        def make_streams(items, train):
            gens = []
            for s, mine in enumerate(segments.deal(items, rank, B, n_streams)):
                def hook(name, s=s):
                    if train:
                        reset_rows.add(s)    # ResetStatesCallback.reset (callbacks.py:50-53)
                generator = windows.segment_windows if isinstance(mine[0], tuple) else windows.file_windows
                gens.append(generator(mine, self.length, self.mapping[0], train=train, repeat=True, rng=rng,
                                      on_new_file=hook, on_unmapped=self._unmapped_input,
                                      char_degradation=self.char_degradation,
                                      context_degradation=self.context_degradation))
            return gens

        def next_batch(gens):
            if isinstance(gens, streams.StreamBatcher):      # B streams advanced together (streams.py)
                batch, rows = gens.next_batch()
                if gens.train:
                    reset_rows.update(rows)                  # ResetStatesCallback.reset (callbacks.py:50-53)
                return batch
            xs, zs, ys = [], [], []
            for g in gens:
                x, z, y = next(g)
                xs.append(x); zs.append(z); ys.append(y)
            return np.stack(xs), np.stack(zs), np.stack(ys)

        def make_batcher(items, train):
            # (an engine with a device assembles the batches there in one launch of its own: HipLM.assemble_windows)
            return streams.StreamBatcher(segments.deal(items, rank, B, n_streams), self.length, self.mapping[0], train=train, rng=rng,
                                         char_degradation=self.char_degradation, context_degradation=self.context_degradation,
                                         on_unmapped=self._unmapped_input, device=getattr(lm, "device", None),
                                         codepoints=getattr(self, "_texts", None),
                                         assembler=getattr(lm, "assemble_windows", None))

        # (the batched path keeps every file's ids in memory -- in HBM for the HIP engine --, 4 bytes per character;
        #  corpora beyond `batched_streams_max_chars` stay on the generator per stream, which re-reads file by file)
        t_phase = time.perf_counter()
        if self.batched_streams and total_size <= self.batched_streams_max_chars:
            train_gens = make_batcher(training_items, True)
            val_gens = make_batcher(validation_items, False)
            train_gens.prepare()
            val_gens.prepare()
            timings['encode'] = time.perf_counter() - t_phase
        else:
            train_gens = make_streams(training_items, True)
            val_gens = make_streams(validation_items, False)
        self._texts = {}
        draw_masks = getattr(lm, "draw_dropout_masks_device", None) if (self.batched_streams and self.device_dropout_masks) else None
        draw_masks = draw_masks or lm.draw_dropout_masks
        steps_per_epoch = max(1, ceil(training_epoch_size / n_streams))
        val_steps = max(1, ceil(validation_epoch_size / n_streams))
        history = {'loss': [], 'accuracy': [], 'val_loss': [], 'val_accuracy': []}
        best_val, best_weights, wait, stopped_epoch = None, None, 0, 0
        self._stop = False
        received = {'n': 0}

        def stopper(sig, _frame):      # StopSignalCallback (callbacks.py:6-34)
            if received['n']:
                self.logger.critical('interrupting')
                raise SystemExit(0)
            self.logger.critical('stopping training')
            received['n'] += 1
            self._stop = True
        try:
            old_handler = signal.signal(signal.SIGINT, stopper)
        except ValueError:             # not in the main thread
            old_handler = None
        nan_abort = False
        try:
            lm.reset_states(B)
            for epoch in range(self.max_epochs):
                t_phase = time.perf_counter()
                lm.read_loss(reset=True)
                loss_sum = acc_sum = 0.0
                # The launches are asynchronous: the next batch is generated on the host while the GPU
                # works on the current one, and only then is the loss read back (a synchronisation).
                # Streams that entered a new file while that batch was generated are reset right before
                # it is trained, as ResetStatesCallback.on_batch_begin does.
                # (the dropout masks of the next step are drawn there too: 2 ms of host work per 1024 streams)
                pending = (next_batch(train_gens), sorted(reset_rows), draw_masks(B))
                reset_rows.clear()
                for step in range(steps_per_epoch):
                    (x, z, y), rows, masks = pending
                    if rows:
                        lm.reset_states(B, rows=rows)
                    # (whatever fails on this rank -- a launch, a timed-out hand-off -- is kept until all ranks have agreed on
                    #  it below: the gradient all-reduce in between is entered by every rank, failed or not)
                    failure = None
                    try:
                        lm.train_window(x, z, y, masks)
                    except Exception as err:
                        failure = err
                    scale = sync.reduce(lm)
                    if failure is None:
                        try:
                            lm.adam_step(grad_scale=scale)
                        except Exception as err:
                            failure = err
                    if step + 1 < steps_per_epoch:
                        pending = (next_batch(train_gens), sorted(reset_rows), draw_masks(B))
                        reset_rows.clear()
                    ce, acc, reg = float('nan'), 0.0, 0.0
                    if failure is None:
                        try:
                            ce, acc, reg = lm.read_loss(reset=True)
                        except Exception as err:      # (a failed hand-off on this rank: every rank must leave together)
                            failure = err
                    loss = ce + reg
                    loss_sum += loss
                    acc_sum += acc
                    if loss > 25:
                        self.logger.warning('huge loss at batch %d', step)
                    # what ends the loop is decided by ALL ranks together: a rank that left on its own would leave
                    # the others waiting in the next all-reduce
                    is_nan, stop, failed = sync.any_flag(not np.isfinite(loss), self._stop, failure is not None)
                    if failed:
                        raise failure if failure is not None else RuntimeError('training failed on another rank')
                    if is_nan:    # TerminateOnNaN
                        self.logger.critical('NaN loss at batch %d', step)
                        nan_abort = True
                        break
                    if stop:
                        self._stop = True
                        break
                history['loss'].append(loss_sum / (step + 1))
                history['accuracy'].append(acc_sum / (step + 1))
                timings['train_steps'] += time.perf_counter() - t_phase
                if nan_abort:
                    break
                t_phase = time.perf_counter()
                # validation: states reset first (callbacks.py:67-69); dropout/regularisers off
                lm.reset_states(B)
                lm.prepare(PREC_BF16)
                v_loss = v_acc = 0.0
                nxt = next_batch(val_gens) if val_steps else None
                v_failure = None
                for k in range(val_steps):
                    x, z, y = nxt
                    try:
                        lm.forward_window(x, z, y, want_probs=False)
                    except Exception as err:
                        v_failure = v_failure or err
                    if k + 1 < val_steps:      # (generated while the GPU works, as in training)
                        nxt = next_batch(val_gens)
                    try:
                        ce, acc, _ = lm.read_loss(reset=True)
                    except Exception as err:
                        v_failure, ce, acc = v_failure or err, float('nan'), 0.0
                    v_loss += ce
                    v_acc += acc
                # (as in the training loop: a rank whose validation failed must not leave the others in the all-reduce below)
                (v_failed,) = sync.any_flag(v_failure is not None)
                if v_failed:
                    raise v_failure if v_failure is not None else RuntimeError('validation failed on another rank')
                v_loss, v_acc = sync.mean_scalars(v_loss / val_steps, v_acc / val_steps)
                history['val_loss'].append(v_loss)
                history['val_accuracy'].append(v_acc)
                lm.reset_states(B)
                timings['validation'] += time.perf_counter() - t_phase
                t_phase = time.perf_counter()
                self.logger.info('epoch %d: loss %.4f accuracy %.4f val_loss %.4f val_accuracy %.4f', epoch + 1,
                                 history['loss'][-1], history['accuracy'][-1], v_loss, v_acc)
                if best_val is None or v_loss < best_val:      # EarlyStopping / ModelCheckpoint
                    best_val, wait = v_loss, 0
                    best_weights = lm.get_weights()
                    if rank == 0:
                        self._checkpoint('ckpt.%02d-%.2f.h5' % (epoch + 1, v_loss))
                else:
                    wait += 1
                    if wait >= self.patience:
                        stopped_epoch = epoch
                        lm.set_weights(best_weights, PREC_BF16)
                        self.logger.info('early stopping at epoch %d, best weights restored', epoch + 1)
                        break
                timings['checkpoint'] += time.perf_counter() - t_phase
                if self._stop:
                    break
        finally:
            if old_handler is not None:
                signal.signal(signal.SIGINT, old_handler)
        self.history = history
        if history['val_loss']:
            self.logger.info('training finished with val_loss %f', min(history['val_loss']))
            if (np.isnan(history['val_loss'][-1]) or stopped_epoch == 0) and best_weights is not None:
                lm.set_weights(best_weights, PREC_BF16)     # rating.py:303-306
            self.status = 2
        else:
            self.logger.critical('training failed')
            self.status = 1

    def _grad_sync(self):
        from .distributed import GradSync
        return GradSync()

    def _checkpoint(self, filename):
        try:
            modelio.save_weights(filename, self.model.get_weights(), self.depth, self.n_ctx)
        except Exception as err:     # checkpoints are best effort
            self.logger.warning('cannot write checkpoint %s: %s', filename, err)

    def print_history(self):
        for k, v in self.history.items():
            print(f"{k}: {v}")

    def _split_data(self, data, val_data):
        '''Read text files, split into training vs validation, count batches and update
        the character mapping (stateful branch of rating.py:317-385).'''
        assert self.status >= 1
        # (the reference shuffles in place with the global `random`; a shuffled index list takes the same swaps, and
        # under data-parallel training every rank must see rank 0's order -- distributed.GradSync)
        order = list(range(len(data)))
        shuffle(order)
        order = self._grad_sync().broadcast_object(order)
        data[:] = [data[i] for i in order]
        if not self.stateful:
            return self._split_data_stateless(data, val_data)
        total_size = 0
        self._texts = {}
        self._sizes = {}      # id(file) -> characters of its normalised text (what segments.plan cuts)
        chars = set(self.mapping[0].keys())
        steps = self.length
        if val_data:
            training_data, validation_data = data, val_data
        else:
            split = ceil(len(data) * self.validation_split)
            training_data, validation_data = data[:-split], data[-split:]
        assert training_data, "stateful mode needs at least one file for training"
        assert validation_data, "stateful mode needs at least one file for validation"
        for file in validation_data:
            self.logger.info('using input %s for validation only', file.name)
        sizes = []
        seen = np.zeros(windows.N_CODEPOINTS, dtype=bool)
        for group in (training_data, validation_data):
            epoch_size = 0
            for file in group:
                file.seek(0)
                text, size = windows.read_normalize_file(file)
                total_size += size
                self._sizes[id(file)] = size
                epoch_size += ceil((size - self.length) / steps / self.batch_size)
                # (the distinct characters through a flag per code point: `set(text)` costs 2.5 ms per 50 k characters;
                #  the code point vectors are what train() maps to ids, it need not read the files again)
                cps = windows.codepoints(text)
                seen[cps] = True
                if self.batched_streams and total_size <= self.batched_streams_max_chars:
                    self._texts[id(file)] = cps
                else:
                    self._texts.clear()
            sizes.append(epoch_size)
        chars.update(chr(int(cp)) for cp in np.nonzero(seen)[0])
        chars = sorted(list(chars))
        self.voc_size = len(chars) + 1
        c_i = dict((c, i) for i, c in enumerate(chars, 1))
        i_c = dict((i, c) for i, c in enumerate(chars, 1))
        self.mapping = (c_i, i_c)
        return training_data, validation_data, None, sizes[0], sizes[1], total_size, steps

    def _split_data_stateless(self, data, val_data):
        '''window-wise split of the stateless mode (rating.py:352-378): windows advance by 3; without
        validation files both generators read the same data and share one uniform number per window
        position that assigns it to training or validation'''
        steps = 3
        total_size, max_size = 0, 0
        chars = set(self.mapping[0].keys())
        for file in data:
            file.seek(0)
            text, size = windows.read_normalize_file(file)
            total_size += size - self.length
            max_size = max(max_size, size)
            chars.update(set(text))
        if val_data:
            training_epoch_size = ceil(total_size / steps / self.batch_size)
            for file in val_data:
                file.seek(0)
                _text, size = windows.read_normalize_file(file)
                total_size += size - self.length
            validation_epoch_size = ceil(total_size / steps / self.batch_size)
            training_data, validation_data, split = data, val_data, None
        else:
            epoch_size = total_size / steps / self.batch_size
            training_epoch_size = ceil(epoch_size * (1 - self.validation_split))
            validation_epoch_size = ceil(epoch_size * self.validation_split)
            validation_data, training_data = data, data
            split = self._grad_sync().broadcast_object(np.random.uniform(0, 1, (ceil(max_size / steps),)))
        if self.first_window:
            training_epoch_size *= 1.0 + self.first_window
        chars = sorted(list(chars))
        self.voc_size = len(chars) + 1
        self.mapping = (dict((c, i) for i, c in enumerate(chars, 1)), dict((i, c) for i, c in enumerate(chars, 1)))
        return training_data, validation_data, split, training_epoch_size, validation_epoch_size, total_size, steps

    def _stateless_gen(self, files, steps, train, split=None, repeat=False):
        return windows.stateless_file_batches(
            files, self.length, self.mapping[0], steps, repeat=repeat, batch_size=self.batch_size, train=train, split=split,
            validation_split=self.validation_split, variable_length=self.variable_length, first_window=self.first_window,
            char_degradation=self.char_degradation, context_degradation=self.context_degradation,
            on_unmapped=self._unmapped_input)

    @staticmethod
    def _last_targets(x, y):
        tgt = np.full(x.shape, -1, dtype=np.int32)
        tgt[:, -1] = y
        return tgt

    def _train_stateless(self, data, val_data=None):
        '''rating.py:248-310 for stateful=False: batches of `batch_size` windows from zero state, one
        target per window; same epoch / early-stopping / checkpoint control as the stateful loop.
        (Single process: the window-wise split has no per-rank sharding.)'''
        (training_data, validation_data, split, training_epoch_size, validation_epoch_size,
         total_size, steps) = self._split_data(data, val_data)
        self.logger.info('training on %d files / %d batches per epoch / %d character tokens for %d character types',
                         len(training_data), training_epoch_size, total_size, self.voc_size)
        self.reconfigure_for_mapping()
        lm = self.model
        if getattr(lm, "precision", PREC_BF16) != PREC_BF16:
            lm.prepare(PREC_BF16)
        train_gen = self._stateless_gen(training_data, steps, True, split, repeat=True)
        val_gen = self._stateless_gen(validation_data, steps, False, split, repeat=True)
        steps_per_epoch = max(1, int(ceil(training_epoch_size)))
        val_steps = max(1, int(ceil(validation_epoch_size)))
        history = {'loss': [], 'accuracy': [], 'val_loss': [], 'val_accuracy': []}
        best_val, best_weights, wait, stopped_epoch = None, None, 0, 0
        nan_abort = False
        for epoch in range(self.max_epochs):
            lm.read_loss(reset=True)
            loss_sum = acc_sum = 0.0
            nxt = next(train_gen)
            for step in range(steps_per_epoch):
                x, z, y = nxt
                b = x.shape[0]
                lm.reset_states(b)
                one = lm.draw_dropout_masks(1)      # noise_shape (1, W): one mask for the whole batch (rating.py:150)
                lm.train_window(x, z, self._last_targets(x, y), np.repeat(one, b, axis=1))
                lm.adam_step()
                if step + 1 < steps_per_epoch:      # the next batch is generated while the GPU works (as in train)
                    nxt = next(train_gen)
                ce, acc, reg = lm.read_loss(reset=True)
                loss = ce + reg
                loss_sum += loss
                acc_sum += acc
                if not np.isfinite(loss):
                    self.logger.critical('NaN loss at batch %d', step)
                    nan_abort = True
                    break
            history['loss'].append(loss_sum / (step + 1))
            history['accuracy'].append(acc_sum / (step + 1))
            if nan_abort:
                break
            lm.prepare(PREC_BF16)
            v_loss = v_acc = 0.0
            n_rows = 0
            nxt = next(val_gen)
            for k in range(val_steps):
                x, z, y = nxt
                b = x.shape[0]
                lm.reset_states(b)
                lm.forward_window(x, z, self._last_targets(x, y), want_probs=False)
                if k + 1 < val_steps:
                    nxt = next(val_gen)
                ce, acc, _ = lm.read_loss(reset=True)
                v_loss += ce * b
                v_acc += acc * b
                n_rows += b
            v_loss, v_acc = v_loss / n_rows, v_acc / n_rows
            history['val_loss'].append(v_loss)
            history['val_accuracy'].append(v_acc)
            self.logger.info('epoch %d: loss %.4f accuracy %.4f val_loss %.4f val_accuracy %.4f', epoch + 1,
                             history['loss'][-1], history['accuracy'][-1], v_loss, v_acc)
            if best_val is None or v_loss < best_val:
                best_val, wait = v_loss, 0
                best_weights = lm.get_weights()
                self._checkpoint('ckpt.%02d-%.2f.h5' % (epoch + 1, v_loss))
            else:
                wait += 1
                if wait >= self.patience:
                    stopped_epoch = epoch
                    lm.set_weights(best_weights, PREC_BF16)
                    self.logger.info('early stopping at epoch %d, best weights restored', epoch + 1)
                    break
        self.history = history
        if history['val_loss']:
            self.logger.info('training finished with val_loss %f', min(history['val_loss']))
            if (np.isnan(history['val_loss'][-1]) or stopped_epoch == 0) and best_weights is not None:
                lm.set_weights(best_weights, PREC_BF16)
            self.status = 2
        else:
            self.logger.critical('training failed')
            self.status = 1

    def reconfigure_for_mapping(self):
        '''Reconfigure the character embedding after a change of mapping, transferring
        previous weights (rating.py:387-414).'''
        assert self.status >= 1
        old_voc = self.model.voc_size if self.model is not None else 0
        if old_voc < self.voc_size:
            if self.status >= 2 and self.model is not None:
                self.logger.warning('transferring weights from previous model with only %d character types', old_voc)
                old = self.model.get_weights()
                self.configure()
                new = self.model.get_weights()
                for name, value in old.items():
                    if name == 'E':
                        new['E'][0:old_voc, :] = value
                    else:
                        new[name] = value
                self.model.set_weights(new)
            else:
                self.configure()

    def remove_from_mapping(self, char=None, idx=None):
        '''Remove one character from mapping and shrink the embedding (rating.py:416-460).'''
        assert self.status > 1
        assert self.voc_size > 0
        if not char and not idx:
            return False
        if char:
            if char in self.mapping[0]:
                idx = self.mapping[0][char]
            else:
                self.logger.error('unmapped character "%s" cannot be removed', char)
                return False
        else:
            if idx in self.mapping[1]:
                char = self.mapping[1][idx]
            else:
                self.logger.error('unmapped index "%d" cannot be removed', idx)
                return False
        weights = self.model.get_weights()
        precision = getattr(self.model, "precision", PREC_SPLIT) or PREC_SPLIT
        self.logger.warning('pruning character "%s" [%d] with norm %f', char, idx, np.linalg.norm(weights['E'][idx, :]))
        c_i, i_c = self.mapping
        c_i.pop(char)
        i_c.pop(idx)
        for i in range(idx + 1, self.voc_size):
            other = i_c.pop(i)
            c_i[other] -= 1
            i_c[i - 1] = other
        self.voc_size -= 1
        weights['E'] = np.delete(weights['E'], idx, 0)
        self.configure()
        self.model.set_weights(weights, precision)
        self.status = 2
        return True

    # ------------------------------------------------------------------ windowed inference
    def _unmapped_input(self, char, position):
        self.logger.error('unmapped character "%s" at input position %d', char, position)

    def _ensure_precision(self):
        lm = self.model
        if getattr(lm, "precision", PREC_SPLIT) != PREC_SPLIT:
            lm.prepare(PREC_SPLIT)

    def test(self, test_data):
        '''Evaluate model on text files: exp(mean cross-entropy) (rating.py:462-491).'''
        assert self.status > 1
        assert self.incremental is False
        self._ensure_precision()
        lm = self.model
        if not self.stateful:
            # one window per character; the batch losses are averaged weighted by batch size, and only
            # ceil((size-1)/batch_size) generator batches per file are evaluated (rating.py:482-490)
            epoch_size = 0
            for file in test_data:
                file.seek(0)
                _text, size = windows.read_normalize_file(file)
                epoch_size += ceil((size - 1) / self.batch_size / 1)
            gen = self._stateless_gen(test_data, 1, False)
            lm.read_loss(reset=True)
            total, rows = 0.0, 0
            for _ in range(epoch_size):
                x, z, y = next(gen)
                lm.reset_states(x.shape[0])
                lm.forward_window(x, z, self._last_targets(x, y), want_probs=False)
                total += lm.read_loss(reset=True)[0] * x.shape[0]
                rows += x.shape[0]
            return exp(total / max(rows, 1))
        lm.reset_states(1)
        lm.read_loss(reset=True)
        n = 0
        total = 0.0
        for x, z, y in windows.file_windows(test_data, self.length, self.mapping[0], on_unmapped=self._unmapped_input):
            lm.forward_window(x[None], z[None], y[None], want_probs=False)
            n += 1
            if n % 64 == 0:
                total += lm.read_loss(reset=True)[0]
        total += lm.read_loss(reset=True)[0]
        return exp(total / max(n, 1))

    def rate(self, text, context=None):
        '''Rate a string all at once (rating.py:493-529): probability of every
        character given its predecessors; the first character gets 1.0.  The
        implicit LSTM state is NOT reset and is advanced over the zero-padded tail
        of the last window, exactly as the reference does.'''
        assert self.status > 1
        assert self.incremental is False
        if not context:
            context = self.underspecify_contexts()
        self._ensure_precision()
        text = windows.normalize(text)
        size = len(text)
        preds = []
        if not self.stateful:
            # Stateless scoring as the reference does it (rating.py:513-528): one window per character
            # position, of which only ceil((size-1)/batch_size) generator batches are evaluated -- the
            # partial windows of the first `length` positions count as batches of their own -- and
            # prediction k (made FOR character k) is paired with character k+1.  Both are reproduced.
            gen = windows.stateless_batches(text, context, self.length, self.mapping[0], 1, batch_size=self.batch_size,
                                            train=False, variable_length=self.variable_length,
                                            on_unmapped=self._unmapped_input)
            for _ in range(ceil((size - 1) / self.batch_size / 1)):
                x, z, _y = next(gen)
                self.model.reset_states(x.shape[0])
                preds.append(_np(self.model.forward_window(x, z))[:, -1])
        for x, z, _y in (windows.stateful_windows(text, context, self.length, self.mapping[0],
                                                  on_unmapped=self._unmapped_input) if self.stateful else ()):
            preds.append(_np(self.model.forward_window(x[None], z[None]))[0])
        probs = [1.0]
        if not preds:
            return probs[:size]
        preds = np.concatenate(preds, axis=0)[0:size]
        for pred, next_char in zip(preds, list(text[1:])):
            idx = self.mapping[0].get(next_char, 0)
            probs.append(pred[idx])
            if len(probs) >= size:
                break
        return probs

    def rate_batch(self, texts, contexts=None, streams=64, want_probs=True, precision="split"):
        '''Rate many INDEPENDENT texts at once: `probs[i]` (float32 array, one entry per character of the normalised
        text) is what `self.model.reset_states(1); self.rate(texts[i], contexts[i])` returns, `bits[i]` (float64) is
        -sum(log2(max(p, 1e-99))) over `probs[i][1:]`; both in input order.  contexts: None, one context list for all
        texts, or one per text.  Up to `streams` texts share a window call, one per row (ratebatch.py); the HIP engine
        delivers one float per character (`rate_window`), or -- want_probs=False, which returns (None, bits) -- one
        double per text.  Unlike `rate`, a batch call neither continues the implicit state of earlier `rate` calls
        nor leaves one behind: afterwards the state is a freshly reset single row.

        precision: "split" (default) rates in the split-precision inference kernels, ~f32 accuracy.  "bf16" is bulk rating
        for whole corpora: the windows run on the bf16 training forward (`rate_window_bulk`: thousands of streams per
        launch; probabilities within 1e-2 of the reference instead of 1e-3), the ids of all texts and the whole plan are
        uploaded once (ratebulk.py), short texts run in windows as short as they are, and with want_probs=False only the
        bits leave the device.  Same return contract; a stateless rater raises ValueError.  The next split-precision
        call restores split precision by itself.'''
        texts, contexts = self._rating_request("rate_batch", texts, contexts, precision)[:2]
        n = len(texts)
        lm = self.model
        if precision == "bf16" and hasattr(lm, 'rate_window_bulk'):
            # (an engine without rate_window_bulk -- the tests' CPU double -- runs the ordinary plan)
            plan, arrays, bits = self._rate_in_corpus_order(texts, contexts, 0, streams, "bf16")
            if not want_probs:
                return None, bits
            if arrays is None:
                return [np.ones(int(m), dtype=np.float32) for m in plan.sizes], bits
            flat = _np(arrays[0])
            return [flat[int(plan.offsets[i]):int(plan.offsets[i + 1])].copy() for i in range(n)], bits
        self._ensure_precision()
        bits = np.zeros(n, dtype=np.float64)
        if not self.stateful:
            # (the stateless rater's windows are batches of 128 already: the loop itself)
            probs = []
            for text, context in zip(texts, contexts):
                probs.append(np.asarray(self.rate(text, context), dtype=np.float32))
            bits[:] = [ratebatch.bits_of(p) for p in probs]
            lm.reset_states(1)
            return (probs if want_probs else None), bits
        texts = [windows.normalize(t) for t in texts]
        ids = [windows.encode(t, self.mapping[0], self._unmapped_input) for t in texts]
        plan = ratebatch.plan(ids, [windows.clamp_context(c) for c in contexts], self.length, streams)
        if plan is None:       # (nothing but empty texts and single characters)
            lm.reset_states(1)
            return ([np.ones(len(t), dtype=np.float32) for t in texts] if want_probs else None), bits
        lm.reset_states(plan.B)
        picked = self._run_plan(plan, 0, bits, want_probs)
        lm.reset_states(1)
        if not want_probs:
            return None, bits
        return [plan.text_probs(i, picked[0]) for i in range(n)], bits

    def _rating_request(self, method, texts, contexts, precision, k=None, max_prob=None, min_rank=None):
        '''What `rate_batch`, `rate_alternatives`, `suspects` and `corrections` (`method`) check of a request before they rate:
        returns (texts as a list, one context list per text, k, np.float32(max_prob), min_rank) -- the last three None where
        the method has no such argument (k: rate_batch; max_prob and min_rank: all but suspects and corrections).'''
        assert self.status > 1
        assert self.incremental is False
        if precision not in ("split", "bf16"):
            raise ValueError('precision must be "split" or "bf16" (got %r)' % (precision,))
        if not self.stateful:
            if min_rank is not None:
                raise ValueError('%s needs a stateful rater: it rates through stateful windows' % method)
            if precision == "bf16":
                raise ValueError('%s(precision="bf16") needs a stateful rater: bulk rating runs stateful windows' % method)
            assert k is None, "%s needs a stateful rater" % method
        limit = None
        if k is not None:
            k = int(k)
            assert 1 <= k <= ratebatch.ALTS_MAX, "k must be in 1..%d" % ratebatch.ALTS_MAX
        if min_rank is not None:
            min_rank, limit = int(min_rank), np.float32(max_prob)
            if min_rank < 0:
                raise ValueError("min_rank must be >= 0 (got %d): a character without a prediction is no suspect" % min_rank)
            if np.isnan(limit):
                raise ValueError("max_prob must not be NaN")
        texts = list(texts)
        return texts, self._contexts_per_text(contexts, len(texts)), k, limit, min_rank

    def _run_plan(self, plan, k, bits, want_probs=True):
        '''The window calls of a ratebatch.Plan (its states reset to plan.B rows by the caller): rows that start a text are
        reset, every call is rated, `bits` (per text) is filled.  Returns the host arrays [picked [n_calls][B][T]] (k == 0;
        None on the HIP engine without want_probs) or [picked, alt_id, alt_p, rank] (k > 0; alt_id, alt_p [n_calls][B][T][k]).
        The HIP engine delivers per call what `rate_window` / `rate_window_alts` return and takes a text's bits from the
        device's f64 sums where it ends, one transfer of each at the end; an engine without these calls (the tests' CPU
        double) delivers the whole softmax of `forward_window`, picked from on the host.'''
        lm = self.model
        device = hasattr(lm, 'rate_window_alts' if k else 'rate_window')
        taken = []
        if device:
            lm.rate_bits_read(reset=True)

            def rate(s, x, z, y):
                out = lm.rate_window_alts(x, z, y, k) if k else (lm.rate_window(x, z, y, want_probs=want_probs),)
                ending = plan.ending(s)
                if ending:       # (a row's sum belongs to the text that ends here: take it, the next text starts from zero)
                    taken.append((ending, lm.rate_bits_take([int(plan.row[i]) for i in ending])))
                return out
        else:
            def rate(s, x, z, y):
                full = _np(lm.forward_window(x, z, want_probs=True))
                return ratebatch.alternatives_of(full, y, k) if k else (_target_probs(full, y),)
        steps = []
        for s in range(plan.n_calls):
            x, z, y = plan.call(s)
            if s and plan.starting(s):
                lm.reset_states(rows=plan.reset_rows(s))
            steps.append(rate(s, x, z, y))
        if device:
            bits[np.concatenate([e for e, _ in taken])] = _np(lm.torch.cat([t for _, t in taken]))
            lm.rate_status_check()
            if not want_probs:
                return None
            return [_np(lm.torch.stack([st[j] for st in steps])) for j in range(len(steps[0]))]
        cols = [np.stack([st[j] for st in steps]) for j in range(len(steps[0]))]
        cols[0] = cols[0].astype(np.float32)
        if k:
            cols[2] = cols[2].astype(np.float32)
        bits[:] = [ratebatch.bits_of(plan.text_probs(i, cols[0])) for i in range(len(bits))]
        return cols

    def _row_costs(self, precision):
        '''How `corrections` and `rescore` rate hypothesis rows: returns rate(x, z, y) -> costs [rows], which runs one window
        from the states as they are.  A row's cost is -sum log2(max(p, 1e-99)), in f64, over its targets.  On the HIP engine
        that is one `rate_window_bulk` ("bf16") or `rate_window` ("split") without probabilities, and the rows' f64 bits are
        the costs (a DEVICE tensor; the caller has cleared the sums before its first window); an engine without these sums
        (the tests' CPU double) delivers the whole softmax of `forward_window`, and the logs are summed on the host.  Which
        form rates is decided here alone, whoever built the windows: `corrections` and `rescore` pick their builders by
        `variant_windows` and `span_windows`, and an engine with the sums rates host-built windows through them too.'''
        lm = self.model
        if hasattr(lm, 'rate_bits_take_all'):
            window = lm.rate_window_bulk if precision == "bf16" else lm.rate_window

            def rate(x, z, y):
                window(x, z, y, want_probs=False)
                return lm.rate_bits_take_all()
        else:
            def rate(x, z, y):
                p = _target_probs(_np(lm.forward_window(x, z, want_probs=True)).astype(np.float64), y)
                return -np.where(y >= 0, np.log2(np.maximum(p, 1e-99)), 0.0).sum(axis=1)
        return rate

    def _span_row_costs(self, source, spans, chunks, precision, left, ahead, M, T):
        '''The chunk loop of `rescore` and `consensus`: the hypothesis rows of `chunks` (`ratebulk.span_chunks`: all S + C rows
        of the spans, in order) built, rated from zero states and their costs gathered.  source = [corpus, offsets, text_ctx or
        None] and spans = [span_text, span_start, span_len, span_first, pool, cand_off] are DEVICE tensors on the HIP engine --
        one `span_windows`, one `reset_states` and one window of `_row_costs` per chunk, the rows' f64 bits into one device
        array, no synchronisation -- and host arrays on an engine without `span_windows` (the tests' CPU double), which runs
        `ratebulk.span_windows_host`.  Returns (cost f64 [S + C], valid int32 [S + C]), device tensors or arrays alike.'''
        lm = self.model
        rate = self._row_costs(precision)
        if hasattr(lm, 'span_windows'):
            torch = lm.torch
            rows = chunks[-1][1]
            cost_d = torch.empty(rows, dtype=torch.float64, device=lm.device)
            valid_d = torch.empty(rows, dtype=torch.int32, device=lm.device)
            lm.rate_bits_read(reset=True)
            for a, b in chunks:
                x, z, y, ok = lm.span_windows(*(list(source) + list(spans)), row0=a, rows=b - a, left=left, ahead=ahead, max_len=M, T=T)
                lm.reset_states(b - a)
                cost_d[a:b] = rate(x, z, y)
                valid_d[a:b] = ok
            return cost_d, valid_d
        costs, valids = [], []
        for a, b in chunks:
            x, z, y, ok = ratebulk.span_windows_host(*(list(source) + list(spans)), a, b - a, left, ahead, M, T)
            lm.reset_states(b - a)
            costs.append(rate(x, z, y))
            valids.append(ok)
        return np.concatenate(costs), np.concatenate(valids)

    def _spans_request(self, method, texts, items):
        '''What `rate_segments` and `rescore` (`method`) check of their spans: items is a sequence whose entries start with
        (i, start, end), [start, end) a span of the NFC-normalised texts[i].  Returns (the normalised texts, offsets [n + 1] of
        their sizes, span_text [S], starts [S], ends [S]), the arrays int64.  ValueError for a text index out of range, a span
        outside its text or with end < start.'''
        texts = [windows.normalize(t) for t in texts]
        n, S = len(texts), len(items)
        sizes = np.asarray([len(t) for t in texts], dtype=np.int64)
        span_text, starts, ends = (np.asarray([int(e[k]) for e in items], dtype=np.int64).reshape(S) for k in range(3))
        outside = (span_text < 0) | (span_text >= n)
        if outside.any():
            raise ValueError("%s: text index %d out of range" % (method, span_text[outside][0]))
        bad = np.nonzero((starts < 0) | (ends < starts) | (ends > sizes[span_text]))[0]
        if len(bad):
            raise ValueError("%s: span [%d, %d) outside text %d of %d characters"
                             % (method, starts[bad[0]], ends[bad[0]], span_text[bad[0]], sizes[span_text[bad[0]]]))
        return texts, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), span_text, starts, ends

    def rate_alternatives(self, texts, contexts=None, k=3, streams=64, precision="split"):
        '''`rate_batch` answering also what the model expected instead: returns (rated, bits), both in input order.
        `rated[i]` is a RatedText over the n characters of the normalised text: `probs` [n] f32 -- what `rate_batch` returns
        for that text --, `alt_ids` [n,k] i32 and `alt_probs` [n,k] f32 -- the k most probable characters at that position,
        ordered by (probability descending, id ascending), padded with -1 / 0 beyond the vocabulary --, and `rank` [n] i32,
        the position of the character that was written in that order (0: the model's first choice).  The first character
        has no prediction: probability 1.0, rank -1, ids -1, probabilities 0.  `bits[i]`, texts, contexts, streams and the
        state afterwards (a freshly reset single row) are as in `rate_batch`.  1 <= k <= 8.  Only stateful raters: the
        stateless one rates through windows of its own (`rate`).

        precision: "split" (default) rates in the split-precision inference kernels.  "bf16" is `rate_batch`'s bulk path
        with alternatives (`rate_window_alts_bulk`, `rate_scatter_alts`): the same plan (ratebulk.py), one upload, the
        results kept in corpus order on the device -- (8k + 8) bytes per character -- and one transfer at the end; `probs`
        are bit for bit those of `rate_batch(precision="bf16")`.  Same return contract; a stateless rater raises
        ValueError; the state and precision afterwards are as after `rate_batch(precision="bf16")`.'''
        texts, contexts, k = self._rating_request("rate_alternatives", texts, contexts, precision, k)[:3]
        n = len(texts)
        if precision == "bf16" and hasattr(self.model, 'rate_window_alts_bulk'):
            # (an engine without rate_window_alts_bulk -- the tests' CPU double -- runs the ordinary path below)
            plan, arrays, bits = self._rate_in_corpus_order(texts, contexts, k, streams, "bf16")
            if arrays is None:
                return [ratebatch.RatedText.unpredicted(int(m), k) for m in plan.sizes], bits
            probs, rank, alt_id, alt_p = (_np(a) for a in arrays)
            cut = [(int(plan.offsets[i]), int(plan.offsets[i + 1])) for i in range(n)]
            return [ratebatch.RatedText(probs[a:b].copy(), rank[a:b].copy(), alt_id[a:b].copy(), alt_p[a:b].copy())
                    for a, b in cut], bits
        self._ensure_precision()
        lm = self.model
        bits = np.zeros(n, dtype=np.float64)
        texts = [windows.normalize(t) for t in texts]
        ids = [windows.encode(t, self.mapping[0], self._unmapped_input) for t in texts]
        plan = ratebatch.plan(ids, [windows.clamp_context(c) for c in contexts], self.length, streams)
        if plan is None:       # (nothing but empty texts and single characters)
            lm.reset_states(1)
            return [ratebatch.RatedText.unpredicted(len(t), k) for t in texts], bits
        lm.reset_states(plan.B)
        picked, alt_id, alt_p, rank = self._run_plan(plan, k, bits)
        lm.reset_states(1)
        return [ratebatch.RatedText(*plan.text_alternatives(i, picked, rank, alt_id, alt_p)) for i in range(n)], bits

    def _rate_in_corpus_order(self, texts, contexts, k, streams, precision, keep=None):
        '''The bulk plan (ratebulk.plan: rows reused, short texts in short windows) over texts with one context list each
        (`_contexts_per_text`), everything kept on the device: one upload (ids, plan rows, reset masks and offsets of all
        calls), per call assemble_windows -> the window call -> a scatter, then one rate_text_bits.  k == 0: probabilities only (rate_window_bulk for "bf16", rate_window for "split" -- the inference
        workspace --, rate_scatter); k > 0: with alternatives (rate_window_alts_bulk or rate_window_alts, rate_scatter_alts).
        Returns (plan, DEVICE tensors in corpus order, bits): (probs [n],) or (probs [n], rank [n], alt_id [n,k], alt_p [n,k]);
        None instead of the tensors if no text has a prediction.  A text's first character keeps 1.0 / -1 / -1 / 0.  A dict
        passed as `keep` receives what stays on the device for a caller that goes on there (`corrections`): corpus (int32
        [n]), offsets (int64 [n_texts + 1]) and text_ctx (int32 [n_texts, n_ctx], the clamped contexts of every text).'''
        lm = self.model
        torch = lm.torch
        n = len(texts)
        texts = [windows.normalize(t) for t in texts]
        ids = [windows.encode(t, self.mapping[0], self._unmapped_input) for t in texts]
        plan = ratebulk.plan([len(a) for a in ids], [windows.clamp_context(c) for c in contexts], self.length, streams)
        bits = np.zeros(n, dtype=np.float64)
        if precision == "split":
            self._ensure_precision()
        if not plan.calls:       # (nothing but empty texts and single characters)
            lm.reset_states(1)
            return plan, None, bits
        n_ctx = plan.n_ctx
        corpus = torch.from_numpy(np.concatenate(ids).astype(np.int32)).to(lm.device)
        rows = torch.from_numpy(np.concatenate([c.rows for c in plan.calls])).to(lm.device)
        reset = torch.from_numpy(np.concatenate([c.reset for c in plan.calls])).to(lm.device)
        offsets = torch.from_numpy(plan.offsets).to(lm.device)
        if keep is not None:
            text_ctx = np.asarray([windows.clamp_context(c) for c in contexts], dtype=np.int32).reshape(n, n_ctx)
            keep.update(corpus=corpus, offsets=offsets, text_ctx=torch.from_numpy(text_ctx).to(lm.device))
        out = [torch.ones(plan.total, dtype=torch.float32, device=lm.device)]      # (1.0: a text's first character)
        if k:      # (rank, alt_id, alt_p)
            out += [torch.full((plan.total,), -1, dtype=torch.int32, device=lm.device),
                    torch.full((plan.total, k), -1, dtype=torch.int32, device=lm.device),
                    torch.zeros((plan.total, k), dtype=torch.float32, device=lm.device)]
        bulk = precision == "bf16"

        def deliver(s, a, b, x, z, y):
            if k:
                p, ai, ap, rk = (lm.rate_window_alts_bulk if bulk else lm.rate_window_alts)(x, z, y, k)
                lm.rate_scatter_alts(p, rk, ai, ap, rows[a:b], n_ctx, *out)
            else:
                p = (lm.rate_window_bulk if bulk else lm.rate_window)(x, z, y, want_probs=True)
                lm.rate_scatter(p, rows[a:b], n_ctx, out[0])
        self._corpus_calls(plan.calls, corpus, rows, reset, n_ctx, deliver)
        bits[:] = _np(lm.rate_text_bits(out[0], offsets))
        lm.rate_bits_read(reset=True)      # (the per-stream sums are not used here; also raises on a timed-out scan hand-off)
        lm.reset_states(1)
        return plan, tuple(out), bits

    def _corpus_calls(self, calls, corpus, rows, reset, n_ctx, deliver):
        '''The window calls of a bulk plan (ratebulk.Call) over an uploaded corpus, in order: rows and reset are the DEVICE
        concatenations of the calls' plan rows and reset masks.  Before a call the rows that start a text are zeroed (all of
        them where the number of rows changes), `assemble_windows` makes its batch, and deliver(s, a, b, x, z, y) rates it and
        takes its results away -- rows[a:b] are the call's.'''
        lm = self.model
        bounds = np.concatenate([[0], np.cumsum([c.B for c in calls])])
        B = None
        for s, call in enumerate(calls):
            a, b = int(bounds[s]), int(bounds[s + 1])
            if call.B != B:
                B = call.B
                lm.reset_states(B)      # (another number of rows: all of them start from zero)
            elif call.reset.any():
                lm.reset_states_where(reset[a:b])
            x, z, y = lm.assemble_windows(corpus, rows[a:b], call.T, n_ctx)
            deliver(s, a, b, x, z, y)

    def rate_contexts(self, texts, candidates, prior=None, streams=1024, precision="bf16", want_probs=True):
        '''Which context does every text read like?  Rates all texts under each of C candidate contexts at once and returns
        one ratebatch.ContextRating per text, in input order: `bits` [C] -- what `rate_batch(texts, contexts=candidates[c])`
        gives for the text --, `posterior` [C] (the prior times 2**-bits, normalised), `best` (an index into `candidates`:
        the most probable one, the smallest among equal ones), `margin` (bits between it and the next candidate of positive
        prior, +inf if there is none), `mix_bits`, and `probs` [n] f32: per character the probability under the sequential
        Bayesian mixture of the candidates -- at every character each candidate weighs as much as its prior times the
        probability it gave to the text so far -- with 1.0 for the first; the rating of a text whose context is not known,
        instead of context 0.  With want_probs=False `probs` is None and nothing per character leaves the device.

        candidates: 1 .. 256 context lists of the model's arity (clamped as everywhere; duplicates are allowed and tie).
        prior: None (uniform) or C non-negative weights with a positive sum; a candidate of weight 0 is rated -- its `bits`
        are delivered -- but takes no part in posterior, best, margin or the mixture.

        On the HIP engine the n * C pairs of a text and a candidate are the rows of ONE bulk plan over one upload of the ids
        (ratebulk.plan_candidates: 64 documents under 20 candidates fill a launch as 1280 streams): per call
        `assemble_windows`, `rate_window_bulk` ("bf16") or `rate_window` ("split"), `rate_scatter_planes` into a [C][characters]
        array, then one `context_mix`.  Texts go in input order in chunks of whole texts of at most ratebulk.PLANE_BYTES of
        that array (a single larger text is a chunk of its own).  An engine without these calls rates once per candidate
        through `rate_batch` and mixes in numpy (ratebulk.context_mix_host).  ValueError for a bad precision, a stateless
        rater with "bf16", no candidate or more than 256, a candidate of another arity, a prior of another length, with a
        negative or non-finite weight or without a positive one.  State and precision afterwards are as after `rate_batch`.'''
        texts = self._rating_request("rate_contexts", texts, None, precision)[0]
        candidates = [list(c) for c in candidates]
        C = len(candidates)
        if not 1 <= C <= ratebulk.CTX_CAND_MAX:
            raise ValueError("rate_contexts: 1 .. %d candidate contexts (got %d)" % (ratebulk.CTX_CAND_MAX, C))
        for c in candidates:
            if len(c) != self.n_ctx:
                raise ValueError("rate_contexts: the model has %d context variables (got %r)" % (self.n_ctx, c))
        candidates = [windows.clamp_context(c) for c in candidates]
        log2prior = None
        if prior is not None:
            weights = np.asarray(prior, dtype=np.float64).reshape(-1)
            if len(weights) != C or not np.isfinite(weights).all() or (weights < 0).any() or not weights.sum() > 0:
                raise ValueError("rate_contexts: prior must be %d non-negative weights with a positive sum" % C)
            with np.errstate(divide="ignore"):
                log2prior = np.log2(weights / weights.sum())
        n = len(texts)
        lm = self.model
        found = [None] * n
        if not self.stateful or not (hasattr(lm, 'rate_scatter_planes') and hasattr(lm, 'context_mix')):
            # a stateless rater (its windows are `rate`'s own), or an engine without the device path (the tests' CPU double):
            # rate_batch per candidate, the numpy statement
            per = [self.rate_batch(texts, candidates[c], streams=streams, precision=precision)[0] for c in range(C)]
            offsets = np.concatenate([[0], np.cumsum([len(p) for p in per[0]])]).astype(np.int64)
            planes = np.ones((C, max(int(offsets[-1]), 1)), dtype=np.float32)
            for c in range(C):
                planes[c, :int(offsets[-1])] = np.concatenate(per[c]) if n else []
            mix = np.ones(planes.shape[1], dtype=np.float32)
            results = ratebulk.context_mix_host(planes, offsets, log2prior, mix if want_probs else None)
            self._context_ratings(found, 0, offsets, results, mix if want_probs else None)
            return found
        torch = lm.torch
        texts = [windows.normalize(t) for t in texts]
        ids = [windows.encode(t, self.mapping[0], self._unmapped_input) for t in texts]
        sizes = np.asarray([len(a) for a in ids], dtype=np.int64)
        if precision == "split":
            self._ensure_precision()
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(lm.device)
        prior_d = None if log2prior is None else up(log2prior)
        bulk = precision == "bf16"
        for t0, t1 in ratebulk.text_chunks(sizes, ratebulk.PLANE_BYTES // (4 * C)):
            plan, plane = ratebulk.plan_candidates(sizes[t0:t1], candidates, self.length, streams)
            total = max(plan.total, 1)
            if not plan.calls:       # (nothing but empty texts and single characters: the prior)
                planes = np.ones((C, total), dtype=np.float32)
                mix = np.ones(total, dtype=np.float32) if want_probs else None
                self._context_ratings(found, t0, plan.offsets, ratebulk.context_mix_host(planes, plan.offsets, log2prior, mix), mix)
                continue
            n_ctx = plan.n_ctx
            corpus = up(np.concatenate(ids[t0:t1]).astype(np.int32))
            rows = up(np.concatenate([c.rows for c in plan.calls]))
            reset = up(np.concatenate([c.reset for c in plan.calls]))
            plane = up(np.concatenate(plane))
            offsets = up(plan.offsets)
            planes = torch.ones((C, total), dtype=torch.float32, device=lm.device)
            mix = torch.ones(total, dtype=torch.float32, device=lm.device) if want_probs else None      # (1.0: a first character)

            def deliver(s, a, b, x, z, y):
                p = (lm.rate_window_bulk if bulk else lm.rate_window)(x, z, y, want_probs=True)
                lm.rate_scatter_planes(p, rows[a:b], plane[a:b], n_ctx, planes)
            self._corpus_calls(plan.calls, corpus, rows, reset, n_ctx, deliver)
            results = [_np(t) for t in lm.context_mix(planes, offsets, prior_d, mix)]
            lm.rate_bits_read(reset=True)      # (the per-stream sums are not used here; also raises on a timed-out scan hand-off)
            self._context_ratings(found, t0, plan.offsets, results, None if mix is None else _np(mix))
            del planes, mix
        lm.reset_states(1)
        return found

    @staticmethod
    def _context_ratings(found, t0, offsets, results, mix):
        '''found[t0 + i] = the ContextRating of text i of a chunk: results as `context_mix` returns them (host arrays), mix the
        chunk's mixture probabilities in corpus order or None'''
        cand_bits, mix_bits, post, best, margin = results
        for i in range(len(offsets) - 1):
            probs = None if mix is None else np.array(mix[int(offsets[i]):int(offsets[i + 1])], dtype=np.float32)
            found[t0 + i] = ratebatch.ContextRating(cand_bits[i].copy(), post[i].copy(), best[i], margin[i], mix_bits[i], probs)

    @staticmethod
    def _empty_selection(k):
        '''a selection without a suspect, as `rate_select` shapes it: (positions, probs, rank, alt_ids [0,k], alt_probs [0,k])'''
        return [np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.int32),
                np.zeros((0, k), dtype=np.int32), np.zeros((0, k), dtype=np.float32)]

    @staticmethod
    def _selection_per_text(sel, offsets):
        '''A corpus-ordered selection (sel[0]: ascending corpus positions; sel[1:]: arrays with one row per position) cut per
        text: [(positions within the text, copies of its rows of sel[1:] ...)].  Positions ascend: a text's share is one slice.'''
        pos = sel[0]
        lo = np.searchsorted(pos, offsets[:-1], side="left")
        hi = np.searchsorted(pos, offsets[1:], side="left")
        return [[pos[a:b] - offsets[i]] + [f[a:b].copy() for f in sel[1:]] for i, (a, b) in enumerate(zip(lo, hi))]

    def suspects(self, texts, contexts=None, k=3, streams=1024, max_prob=0.01, min_rank=1, precision="bf16"):
        '''Where are the characters the model does not believe, and what would it have written there?  Returns (found, bits),
        both in input order: `found[i]` is a ratebatch.Suspects holding exactly the rows j of
        `rate_alternatives(texts, contexts, k, streams, precision)[0][i]` with rank[j] >= min_rank and
        probs[j] <= np.float32(max_prob), in ascending j (`positions`); `bits` is as in `rate_batch`.  A text's first
        character has no prediction and is never a suspect (min_rank >= 0 is required).

        precision "bf16" (default) rates on the bulk path and picks the suspects out on the device (`rate_select` over the
        whole corpus): what leaves the device is count * (8k + 16) bytes plus the bits.  "split" runs the same plan through
        the split-precision `rate_window_alts`.  Either way the results of ALL texts stay on the device in corpus order
        until the selection: (8k + 8) bytes of device memory per character.  Only stateful raters; the state afterwards is a
        freshly reset single row, the precision that of the path taken.'''
        texts, contexts, k, limit, min_rank = self._rating_request("suspects", texts, contexts, precision, k, max_prob, min_rank)
        lm = self.model
        if not hasattr(lm, 'rate_window_alts_bulk'):
            # an engine without the device path (the tests' CPU double): rate_alternatives' fallback and the numpy statement
            rated, bits = self.rate_alternatives(texts, contexts, k=k, streams=streams, precision=precision)
            found = []
            for one in rated:
                found.append(ratebatch.Suspects(*ratebulk.select_host(one.probs, one.rank, one.alt_ids, one.alt_probs,
                                                                      limit, min_rank)))
            return found, bits
        plan, arrays, bits = self._rate_in_corpus_order(texts, contexts, k, streams, precision)
        if arrays is None:
            sel = self._empty_selection(k)
        else:
            sel = [_np(t) for t in lm.rate_select(*arrays, max_prob=float(limit), min_rank=min_rank)]
        return [ratebatch.Suspects(*one) for one in self._selection_per_text(sel, plan.offsets)], bits

    def _delimiter_table(self, delimiters):
        '''uint8 [voc_size]: 1 at the ids of the characters that separate words -- those of the (normalised) string, or every
        mapped character with str.isspace(); characters outside the mapping have no id of their own and are left out'''
        chars = [c for c in self.mapping[0] if c.isspace()] if delimiters is None else windows.normalize(delimiters)
        table = np.zeros(self.voc_size, dtype=np.uint8)
        for c in chars:
            if 0 < self.mapping[0].get(c, 0) < self.voc_size:
                table[self.mapping[0][c]] = 1
        return table

    def suspect_words(self, texts, contexts=None, delimiters=None, k=3, streams=1024, max_prob=0.01, min_rank=1, min_suspects=1,
                      min_bits_per_char=0.0, min_chars=1, precision="bf16"):
        '''Which WORDS does the model not believe?  `suspects` per word, for whoever looks words up -- a lexicon, a spell
        checker, a second OCR engine's token (`ratebatch.word_edits` makes `rescore`'s edits of them).  Returns (found, bits),
        both in input order: `bits` is as in `rate_batch`, `found[i]` a ratebatch.Words holding, in ascending order, the words
        of the normalised texts[i] with at least `min_chars` predicted characters, at least `min_suspects` suspect characters
        (rank >= min_rank and probability <= np.float32(max_prob), as in `suspects`) and at least `min_bits_per_char` bits per
        predicted character -- with their bits, mean and least probability, the place of the least probable character and the
        number of suspects.

        A word is a maximal run of characters that are no delimiters, within one text.  delimiters is a string; the default is
        every mapped character with str.isspace().  A whitespace character outside the mapping has id 0, as every unmapped
        character has, and is part of a word; so is a character of `delimiters` that is not mapped.  A text's first character
        has no prediction: it belongs to its word (`start`, `length`) but not to the word's ratings (`n`).

        On the HIP engine everything stays on the device in corpus order, as in `suspects`: `word_bounds` finds the words,
        `rate_segments` rates them, `segment_select` picks them out, and 52 bytes per selected word plus the bits leave the
        device; the selection is cut per text on the host (`_words_per_text`: the texts without a word share one empty result).  An engine without `rate_segments` runs `rate_alternatives` and the numpy statements of ratebulk.py.  texts,
        contexts, k, streams and precision are as in `suspects` (k only sizes the rating pass), and so are the state and the
        precision afterwards.  ValueError for a stateless rater, min_suspects < 0, min_chars < 1, a negative or NaN
        min_bits_per_char.'''
        texts, contexts, k, limit, min_rank = self._rating_request("suspect_words", texts, contexts, precision, k, max_prob,
                                                                   min_rank)
        min_suspects, min_chars, min_bpc = int(min_suspects), int(min_chars), float(min_bits_per_char)
        if min_suspects < 0 or min_chars < 1 or not min_bpc >= 0.0:
            raise ValueError("min_suspects >= 0, min_chars >= 1 and min_bits_per_char >= 0 (got %d, %d, %r)"
                             % (min_suspects, min_chars, min_bits_per_char))
        delim = self._delimiter_table(delimiters)
        rule = dict(min_n=min_chars, min_bad=min_suspects, min_bpc=min_bpc)
        lm = self.model
        if not hasattr(lm, 'rate_segments'):
            # an engine without the device path (the tests' CPU double): rate_alternatives and the numpy statements, per text
            rated, bits = self.rate_alternatives(texts, contexts, k=k, streams=streams, precision=precision)
            found = []
            for text, one in zip(texts, rated):
                ids = windows.encode(windows.normalize(text), self.mapping[0])
                offsets = np.asarray([0, len(ids)], dtype=np.int64)
                start, end = ratebulk.word_bounds_host(ids, offsets, delim)
                records = ratebulk.segments_host(one.probs, one.rank, offsets, start, end, limit, min_rank)
                found.append(ratebatch.Words.from_records(*ratebulk.segment_select_host(start, end, *records, **rule)[1:]))
            return found, bits
        keep = {}
        plan, arrays, bits = self._rate_in_corpus_order(texts, contexts, k, streams, precision, keep=keep)
        sel = None
        if arrays is not None:
            start, end = lm.word_bounds(keep["corpus"], keep["offsets"], lm.torch.from_numpy(delim).to(lm.device))
            if start.numel():
                records = lm.rate_segments(arrays[0], arrays[1], keep["offsets"], start, end, float(limit), min_rank)
                sel = [_np(t) for t in lm.segment_select(start, end, records, **rule)[1:]]      # (all but the index)
        if sel is None:
            sel = [np.zeros(0, dtype=kind) for kind in (np.int64, np.int64, np.int32, np.float64, np.float64, np.float32,
                                                        np.int64, np.int32)]
        return self._words_per_text(sel, plan.offsets), bits

    @staticmethod
    def _words_per_text(sel, offsets):
        '''A corpus-ordered selection of words (the records of `segment_select` without the index: start, end, n, bits, psum,
        min, worst, bad; starts ascending) cut per text as `_selection_per_text` cuts: one ratebatch.Words per text.  Positions
        within the texts and the means are taken for the whole selection at once; a text's share is one slice of views, and the
        texts without a word (many lines of a corpus of lines) share ONE empty result, as in `rescore`: the split costs per text
        with a word.'''
        base = offsets[np.searchsorted(offsets, sel[0], side="right") - 1]
        whole = ratebatch.Words.from_records(*sel, offset=base)
        lo = np.searchsorted(sel[0], offsets[:-1], side="left")
        hi = np.searchsorted(sel[0], offsets[1:], side="left")
        found = [whole.cut(0, 0)] * (len(offsets) - 1)
        for i in np.nonzero(hi > lo)[0].tolist():
            found[i] = whole.cut(int(lo[i]), int(hi[i]))
        return found

    def rate_segments(self, texts, segments, contexts=None, streams=1024, precision="bf16"):
        '''How does the model rate these spans of the texts?  The bulk counterpart of the processor's score per TextEquiv
        substring (a mean over the character probabilities of the substring).  segments is a sequence of (i, start, end):
        [start, end) is a span of the NFC-normalised texts[i], as in `rescore`'s edits; spans may overlap.  Returns one
        ratebatch.Segments per text holding that text's spans in the order given (the texts without a span share one empty
        result): bits, mean and least probability and the
        place of the least probable character, over the characters of the span that have a prediction (`n`: all but a text's
        first character; an empty span, or the first character alone, has n 0, bits 0.0, mean NaN, least +inf, worst -1).
        No ranks are computed: `suspects` are zeros.

        On the HIP engine the texts are rated with probabilities only (the bulk plan of `rate_batch(precision="bf16")`, or the
        same plan through `rate_window` for "split"), the probabilities stay on the device in corpus order, `rate_segments`
        reduces them per span, and 36 bytes per span leave the device -- no per-character array does.  An engine without
        `rate_segments` runs `rate_batch` and the numpy statement.  ValueError for a stateless rater, a text index out of
        range, a span outside its text or with end < start.  State and precision afterwards are as after `suspects`.'''
        texts, contexts = self._rating_request("rate_segments", texts, contexts, precision)[:2]
        if not self.stateful:
            raise ValueError('rate_segments needs a stateful rater: it rates through stateful windows')
        n = len(texts)
        segments = list(segments)
        S = len(segments)
        _, offsets, span_text, starts, ends = self._spans_request("rate_segments", texts, segments)
        seg_start, seg_end = starts + offsets[span_text], ends + offsets[span_text]      # (corpus positions)
        lm = self.model
        if not hasattr(lm, 'rate_segments'):
            # an engine without the device path (the tests' CPU double): rate_batch and the numpy statement
            probs, _ = self.rate_batch(texts, contexts, streams=streams, precision=precision)
            flat = np.concatenate([np.zeros(0, dtype=np.float32)] + [np.asarray(p, dtype=np.float32) for p in probs])
            records = ratebulk.segments_host(flat, None, offsets, seg_start, seg_end)
        else:
            keep = {}
            arrays = self._rate_in_corpus_order(texts, contexts, 0, streams, precision, keep=keep)[1] if S else None
            if arrays is None:      # (no span, or no text with a prediction -- which the statement needs no engine for)
                lm.reset_states(1)
                records = ratebulk.segments_host(np.ones(int(offsets[-1]), dtype=np.float32), None, offsets, seg_start, seg_end)
            else:
                up = lambda a: lm.torch.from_numpy(np.ascontiguousarray(a)).to(lm.device)
                records = [_np(t) for t in lm.rate_segments(arrays[0], None, keep["offsets"], up(seg_start), up(seg_end))]
        order = np.argsort(span_text, kind="stable")
        cut = np.searchsorted(span_text[order], np.arange(n + 1), side="left")
        whole = ratebatch.Segments.from_records(seg_start[order], seg_end[order], *[r[order] for r in records],
                                                offset=offsets[span_text[order]])
        # (most texts of a large corpus may hold no span at all: they share ONE empty result, as in `rescore`)
        found = [whole.cut(0, 0)] * n
        for i in np.unique(span_text).tolist():
            found[i] = whole.cut(int(cut[i]), int(cut[i + 1]))
        return found

    def corrections(self, texts, contexts=None, k=3, streams=1024, max_prob=0.01, min_rank=1, left=64, ahead=8, deletions=False,
                    min_gain=1.0, precision="bf16", insertions=False, share_left=False):
        '''`suspects`, and for every suspect: does the text that FOLLOWS read better with one of the model's alternatives than
        with the character that was written?  Returns (found, bits), both in input order; `bits` and texts, contexts, k,
        streams, max_prob, min_rank and precision are as in `suspects`, and `found[i]` is a ratebatch.Corrections: the five
        arrays of `suspects(...)[0][i]`, bit for bit, plus `cost` [m,R] f64, `best_id` [m] i32, `gain` [m] f64 and `best_op`
        [m] i32.

        A suspect at position j of a text of n characters has R = k + 1 + deletions + k * insertions variants: 0 the character
        as written, v = 1 .. k the alternative alt_ids[:, v-1] in its place (no variant where that is -1 or the character
        itself), k + 1 (deletions only) the character dropped (no variant at the text's last character), and (insertions only)
        v = k + 1 + deletions + j, j = 0 .. k-1, the alternative alt_ids[:, j] inserted IN FRONT of the written character -- a
        character the text has lost (no variant where that is -1; the written character doubled is one).  With L = min(left, j)
        and A = min(ahead, n - 1 - j), a variant's cost is -sum log2(max(p, 1e-99)), in f64, over the predictions of its own
        character(s) (none, one, or the inserted and the written one) and the A characters after it, made by a stateful window
        that starts from a ZERO state and has read the L characters in front of the suspect; +inf where there is no such
        variant.  An insertion explains the same written characters as variant 0 under a true text one character longer, as a
        deletion does under one that is shorter.  `best_id` is the id of the variant v >= 1 of least cost (the smallest v among
        equal costs: substitution before deletion before insertion; Corrections.DELETE = -2 for the dropped character),
        `best_op` says which edit it is (Corrections.OP_SUBSTITUTE, OP_DELETE, OP_INSERT) and `gain` = cost[0] - cost[best] in
        bits -- kept only where gain >= min_gain, else Corrections.NO_PROPOSAL = -1, OP_NONE and 0.0.
        `Corrections.apply(text, mapping)` writes the kept proposals into a text, `Corrections.edits` lists them.

        The left context is cut at `left` characters and starts from a zero state: exact for a suspect within the first `left`
        characters of its text, beyond that an approximation -- one that the written variant and its alternatives share, so the
        comparison between them stays fair.  The first-pass alternatives are the model's guess from the left context alone;
        `cost[:, 0]` is therefore NOT derived from `probs`.

        On the HIP engine the id corpus, the text offsets, the contexts and the selection stay on the device; suspects are taken
        in chunks of max(1, streams // R): zero states, `variant_windows` at T = max(left + ahead + insertions, 3), one
        `rate_window_bulk` ("bf16") or `rate_window` ("split"), the rows' f64 bits are the costs.  Beyond the suspects' records
        (8k + 16 bytes each) 12 * R bytes per suspect leave the device.  ValueError for a stateless rater, left < 1, ahead < 0 or
        left + ahead + insertions > 1024.  State and precision afterwards are as after `suspects`.

        share_left=True reads a suspect's left context once for all its R variants instead of once per variant.  The costs
        follow the same definition -- a zero state, the L characters in front, the variant, A characters --, the arithmetic is
        cut in two stateful windows: the suspects with L == left get one prefix row each (`prefix_windows` at T = left - 1, in
        batches of (streams // chunk) * chunk suspects from zero states), and per chunk their variants' rows continue from the
        states these left (`fan_states`, then `variant_windows(left=1)` at T = max(1 + ahead + insertions, 3)).  On the CPU
        double the state only passes through an array, and the costs agree to rounding; on the device the two routes are
        different launches over different numbers of rows and are not held to agree bit for bit -- each is held to the
        definition in its precision.  Only L == left is shared: the suspects within the first `left` characters of their text
        (L < left) run as without the flag, in chunks of their own -- on long texts nearly every suspect is shared, on short
        lines with left = 64 almost none is: choose a smaller `left` there.
        Below left = 4 the prefix window would be shorter than the persistent scans take, and share_left=True runs the
        unshared route, bit for bit.  `shared_left` afterwards is None, or where suspects were shared a dict: suspects, shared
        (those with L == left), prefix_windows, suffix_windows and unshared_windows (the window calls of each kind).'''
        texts, contexts, k, limit, min_rank = self._rating_request("corrections", texts, contexts, precision, k, max_prob,
                                                                    min_rank)
        left, ahead, deletions, insertions = int(left), int(ahead), int(bool(deletions)), int(bool(insertions))
        if left < 1 or ahead < 0 or left + ahead + insertions > 1024:
            raise ValueError("left >= 1, ahead >= 0 and left + ahead%s <= 1024 (got %d, %d)"
                             % (" + 1 (insertions)" if insertions else "", left, ahead))
        n = len(texts)
        lm = self.model
        R = k + 1 + deletions + k * insertions
        chunk = max(1, int(streams) // R)
        T = max(left + ahead + insertions, ratebulk.MIN_T)
        device = hasattr(lm, 'variant_windows')
        share = bool(share_left) and left - 1 >= ratebulk.MIN_T      # (a shorter prefix window would fall off the persistent scans)
        rate = self._row_costs(precision)
        # per path: the suspects (sel, in corpus order; pos and alts where the windows are built), then callables -- `build`
        # makes the variants' windows (idx, ctx, tgt, valid) of some suspects (`rate` runs one from the states as they are and
        # returns its rows' costs); for share_left also `prefix` (the left contexts' windows), `start` (zero states for n prefix
        # rows), `fan` (the states of the rows [lo * R, hi * R) that continue from the prefix rows lo .. hi - 1 of `pre`),
        # `take` (pos and alts of the suspects an index array names) and `place` (rows in the order they were rated, back to
        # corpus order)
        if device:
            keep = {}
            plan, arrays, bits = self._rate_in_corpus_order(texts, contexts, k, streams, precision, keep=keep)
            offsets = plan.offsets
            sel_d = lm.rate_select(*arrays, max_prob=float(limit), min_rank=min_rank) if arrays is not None else None
            del arrays
            S = int(sel_d[0].numel()) if sel_d is not None else 0
            sel = [_np(t) for t in sel_d] if S else self._empty_selection(k)
            cat = lm.torch.cat
            pos, alts = (sel_d[0], sel_d[3]) if S else (None, None)
            source = (keep.get("corpus"), keep.get("offsets"), keep.get("text_ctx") if lm.n_ctx else None)

            def build(pos, alts, left, T):
                return lm.variant_windows(*source, pos, alts, left, ahead, deletions, T, insertions=bool(insertions))

            def prefix(pos):
                return lm.prefix_windows(*source, pos, left, left - 1)

            def start(n, pre):
                # (the last batch's buffer again where it fits: a window's replayed launch sequence is keyed by the address of
                # its states)
                if pre is not None and pre.shape[0] == n:
                    lm.states = pre
                lm.reset_states(n)

            def fan(pre, lo, hi):
                lm.fan_states(pre, lm.torch.arange(lo * R, hi * R, dtype=lm.torch.int32, device=lm.device) // R)

            def take(index):
                index = lm.torch.from_numpy(index).to(lm.device)
                return pos[index], alts[index]

            def place(rows, order):
                out = lm.torch.empty_like(rows)
                out[lm.torch.from_numpy(order).to(lm.device)] = rows
                return out
        else:
            # an engine without the device path (the tests' CPU double): `suspects`, the numpy statement of the windows, the
            # whole softmax of every window and the logs summed on the host
            found, bits = self.suspects(texts, contexts, k=k, streams=streams, max_prob=max_prob, min_rank=min_rank,
                                        precision=precision)
            ids = [windows.encode(windows.normalize(t), self.mapping[0]) for t in texts]
            offsets = np.concatenate([[0], np.cumsum([len(a) for a in ids])]).astype(np.int64)
            sel = [np.concatenate([getattr(f, name) for f in found]) if n else e
                   for name, e in zip(("positions", "probs", "rank", "alt_ids", "alt_probs"), self._empty_selection(k))]
            sel[0] = sel[0] + np.repeat(offsets[:-1], [len(f) for f in found])
            S = len(sel[0])
            cat = np.concatenate
            pos, alts = sel[0], sel[3]
            if S:
                corpus = np.concatenate(ids).astype(np.int32)
                text_ctx = np.asarray([windows.clamp_context(c) for c in contexts], dtype=np.int32).reshape(n, -1)

            def build(pos, alts, left, T):
                return ratebulk.variant_windows_host(corpus, offsets, text_ctx, pos, alts, left, ahead, deletions, T, insertions)

            def prefix(pos):
                return ratebulk.prefix_windows_host(corpus, offsets, text_ctx, pos, left, left - 1)

            def start(n, pre):
                lm.reset_states(n)

            def fan(pre, lo, hi):
                lm.states = ratebulk.fan_states_host(pre, np.arange(lo * R, hi * R) // R)

            def take(index):
                return pos[index], alts[index]

            def place(rows, order):
                out = np.empty_like(rows)
                out[order] = rows
                return out
        costs, valids = [], []

        def unshared(pos, alts):      # suspects in chunks, every variant's window from a zero state
            for a in range(0, len(pos), chunk):
                x, z, y, ok = build(pos[a:a + chunk], alts[a:a + chunk], left, T)
                lm.reset_states(int(x.shape[0]))
                costs.append(rate(x, z, y))
                valids.append(ok)
        self.shared_left = None
        if S and share:
            # the suspects with the whole of `left` characters in front of them: one prefix row each, left - 1 characters from a
            # zero state, then per chunk its variants' short rows (left = 1: x[g-1], the variant, `ahead` characters) from the
            # states the prefix rows left; the others as without share_left
            full, short = ratebulk.left_groups(sel[0], offsets, left)
            batches = ratebulk.prefix_batches(len(full), streams, R)
            self.shared_left = dict(suspects=S, shared=len(full), prefix_windows=len(batches),
                                    suffix_windows=sum(len(chunks) for _, _, chunks in batches),
                                    unshared_windows=-(-len(short) // chunk))
            if len(short):
                unshared(*take(short))
            full_pos, full_alts = take(full) if len(full) else (None, None)
            short_T = max(1 + ahead + insertions, ratebulk.MIN_T)
            pre = None
            for a, b, chunks in batches:
                x, z, y, _ = prefix(full_pos[a:b])
                start(b - a, pre)
                rate(x, z, y)      # (no targets: the bits it adds are zeros)
                pre = lm.states
                for c, d in chunks:
                    x, z, y, ok = build(full_pos[c:d], full_alts[c:d], 1, short_T)
                    fan(pre, c - a, d - a)
                    costs.append(rate(x, z, y))
                    valids.append(ok)
            order = np.concatenate([short, full])
            cost, valid = (_np(place(cat(rows).reshape(S, R), order)) for rows in (costs, valids))
        elif S:
            unshared(pos, alts)
            cost, valid = _np(cat(costs)).reshape(S, R), _np(cat(valids)).reshape(S, R)
        if S:
            if device:
                lm.rate_status_check()
            lm.reset_states(1)
        else:
            cost, valid = np.zeros((0, R), dtype=np.float64), np.zeros((0, R), dtype=np.int32)
        cost, best, gain = ratebulk.variant_pick_host(cost, valid)
        # best v -> edit: 1 .. k substitute alt_ids[v-1]; k + 1 with deletions: delete; from k + 1 + deletions on: insert
        Cor = ratebatch.Corrections
        best_id = np.full(S, Cor.NO_PROPOSAL, dtype=np.int32)
        best_op = np.full(S, Cor.OP_NONE, dtype=np.int32)
        swap = np.nonzero((best >= 1) & (best <= k))[0]
        best_id[swap] = sel[3][swap, best[swap] - 1]
        best_op[swap] = Cor.OP_SUBSTITUTE
        if deletions:
            best_id[best == k + 1] = Cor.DELETE
            best_op[best == k + 1] = Cor.OP_DELETE
        put = np.nonzero(best >= k + 1 + deletions)[0]
        best_id[put] = sel[3][put, best[put] - (k + 1 + deletions)]
        best_op[put] = Cor.OP_INSERT
        with np.errstate(invalid="ignore"):
            drop = (best == 0) | ~(gain >= float(min_gain))
        best_id[drop] = Cor.NO_PROPOSAL
        best_op[drop] = Cor.OP_NONE
        gain[drop] = 0.0
        return [ratebatch.Corrections(*one)
                for one in self._selection_per_text(list(sel) + [cost, best_id, gain, best_op], offsets)], bits

    def rescore(self, texts, edits, contexts=None, streams=1024, left=64, ahead=8, min_gain=1.0, precision="bf16", want_costs=True,
                prior=None):
        '''Does a text read better with one of the caller's replacements for a span of it?  `corrections` for readings that come
        from outside the model -- a second OCR engine, a lexicon, a table of confusions (`ratebatch.confusion_edits`) --, many
        characters for many.  edits is a sequence of (i, start, end, candidates): [start, end) is a span of the NFC-normalised
        texts[i] (end == start: an insertion in front of start), candidates a list of replacement strings, normalised by the
        call and encoded with the rater's mapping; "" drops the span.  Returns `found`, one ratebatch.Rescored per text holding
        that text's spans in the order given (the texts without a span share one empty result).

        With D = end - start, L = min(left, start) and A = min(ahead, n - end) in a text of n characters, the cost of a reading
        r (the span as written, or a candidate) is -sum log2(max(p, 1e-99)), in f64, over the predictions of r and of the A
        characters after the span, made by a stateful window that starts from a ZERO state and has read the L characters in
        front of the span: `corrections`' definition, and its fairness argument -- all readings of a span share the left
        context and the continuation.  +inf where there is no such hypothesis: a span at a text's first character (no
        prediction to be held against: all of it +inf, as a text's first character is never a suspect), a span and continuation
        of no characters at all, a candidate equal to what is written (as ids: two different unmapped characters are equal)
        or, with A == 0, the empty one.  `best` is the candidate of least cost (the first among equal ones), `gain` =
        cost0 - cost[best] in bits -- kept only where gain >= min_gain, else -1 and 0.0.

        On the HIP engine no first pass is run: ids, offsets, contexts, spans and the candidate pool are uploaded once; the
        rows (one per span for the text as written, one per candidate) are taken in chunks of consecutive whole spans of at
        most `streams` rows (a span with more rows is a chunk of its own): zero states, `span_windows` at
        T = max(left + ahead + M - 1, 3) with M the longest span or candidate of the call, one `rate_window_bulk` ("bf16") or
        `rate_window` ("split"), the rows' f64 bits into one device array; at the end one `span_pick`.  With want_costs=False
        only 12 bytes per span leave the device (cost0 and cost are None).  ValueError for a stateless rater, left < 1,
        ahead < 0, a text index out of range, a span outside its text or with end < start, a span or candidate longer than 64
        characters, left + ahead + M - 1 > 1024.  No edits, or only spans that cannot hold a prediction, give their results
        without a launch.  State and precision afterwards are as after `suspects`.

        prior (None: the model's bits alone, the path above with nothing added) is a sequence parallel to `edits` of
        per-candidate bits >= 0 from outside the model -- what a candidate costs under a channel (`correct_words(channel=..)`).
        They are added in f64 to the candidates' rows before the pick, the text as written gets nothing: `cost` then holds
        the sums, `best` and `gain` are taken over them.  On the device that is one add of an uploaded array.  ValueError for
        a prior of another shape than the edits' candidates, or a negative or non-finite value.'''
        texts, contexts = self._rating_request("rescore", texts, contexts, precision)[:2]
        if not self.stateful:
            raise ValueError('rescore needs a stateful rater: it rates through stateful windows')
        left, ahead, streams = int(left), int(ahead), max(1, int(streams))
        if left < 1 or ahead < 0:
            raise ValueError("left >= 1 and ahead >= 0 (got %d, %d)" % (left, ahead))
        n = len(texts)
        lm = self.model
        edits = list(edits)
        S = len(edits)
        count = [len(e[3]) for e in edits]      # (the candidates are read before a span is refused)
        strings = [windows.normalize(c) for e in edits for c in e[3]]
        lengths = np.asarray([len(c) for c in strings], dtype=np.int64)
        C = len(strings)
        texts, offsets, span_text, starts, ends = self._spans_request("rescore", texts, edits)
        sizes = offsets[1:] - offsets[:-1]
        span_text, span_len = span_text.astype(np.int32), (ends - starts).astype(np.int32)
        M = int(max([1] + ([int(span_len.max())] if S else []) + ([int(lengths.max())] if C else [])))
        if M > ratebulk.SPAN_LEN_MAX:
            raise ValueError("rescore: a span or candidate longer than %d characters" % ratebulk.SPAN_LEN_MAX)
        if left + ahead + M - 1 > 1024:
            raise ValueError("left + ahead + %d - 1 <= 1024 (got %d, %d)" % (M, left, ahead))
        T = max(left + ahead + M - 1, ratebulk.MIN_T)
        span_first = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
        prior_rows = None
        if prior is not None:
            prior = [np.asarray(one, dtype=np.float64).reshape(-1) for one in prior]
            if len(prior) != S or any(len(one) != c for one, c in zip(prior, count)):
                raise ValueError("rescore: prior holds one value per candidate of every edit")
            flat = np.concatenate(prior) if prior else np.zeros(0, dtype=np.float64)
            if not (np.isfinite(flat).all() and (flat >= 0.0).all()):
                raise ValueError("rescore: prior values are bits >= 0, finite")
            prior_rows = np.zeros(S + C, dtype=np.float64)      # (candidate c of span s has row c + s + 1)
            prior_rows[np.arange(C, dtype=np.int64) + np.repeat(np.arange(S, dtype=np.int64), count) + 1] = flat
        if precision == "split":
            self._ensure_precision()
        cost = np.full(S + C, np.inf, dtype=np.float64) if want_costs else None
        best = np.full(S, -1, dtype=np.int32)
        gain = np.zeros(S, dtype=np.float64)
        # (a span at a text's first character, and one in a text of a single character, holds no prediction)
        if S and ((starts >= 1) & (sizes[span_text] >= 2)).any():
            # (all texts, and all candidates, encoded in one go: many short strings cost a Python loop each)
            joined = "".join(texts)
            corpus = self._corpus_ids(joined, offsets)
            clamped = {}      # (one context list for all texts is one object n times)
            for c in contexts:
                if id(c) not in clamped:
                    clamped[id(c)] = windows.clamp_context(c)
            text_ctx = np.asarray([clamped[id(c)] for c in contexts], dtype=np.int32).reshape(n, -1)
            span_start = starts + offsets[span_text]      # (corpus positions)
            pool = windows.encode("".join(strings), self.mapping[0]).astype(np.int32)
            cand_off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
            chunks = ratebulk.span_chunks(span_first, streams)
            if hasattr(lm, 'span_windows'):
                torch = lm.torch
                up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(lm.device)
                where = [up(a) for a in (corpus, offsets)] + [up(text_ctx) if lm.n_ctx else None]
                spans = [up(a) for a in (span_text, span_start, span_len, span_first, pool, cand_off)]
                cost_d, valid_d = self._span_row_costs(where, spans, chunks, precision, left, ahead, M, T)
                if prior_rows is not None:
                    cost_d = cost_d + up(prior_rows)
                best_d, gain_d, cost_d = lm.span_pick(cost_d, valid_d, spans[3], float(min_gain), want_costs=want_costs)
                lm.rate_status_check()
                best, gain = _np(best_d), _np(gain_d)
                if want_costs:
                    cost = _np(cost_d)
            else:
                # an engine without the device path (the tests' CPU double): the numpy statements of the windows and of the
                # choice, the whole softmax of every window and the logs summed on the host
                costs, valids = self._span_row_costs([corpus, offsets, text_ctx], [span_text, span_start, span_len, span_first, pool,
                                                                                   cand_off], chunks, precision, left, ahead, M, T)
                if prior_rows is not None:
                    costs = costs + prior_rows
                best, gain, all_costs = ratebulk.span_pick_host(costs, valids, span_first, float(min_gain))
                if want_costs:
                    cost = all_costs
        lm.reset_states(1)
        # per text: its spans in the order given -- everything gathered text by text once, then cut
        order = np.argsort(span_text, kind="stable")
        cut = np.searchsorted(span_text[order], np.arange(n + 1), side="left")
        counts = (span_first[1:] - span_first[:-1])[order]
        first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        # the candidates of the spans in that order: candidate c of span s has row c + s + 1
        cands = np.repeat(span_first[order] - first[:-1], counts) + np.arange(int(first[-1]), dtype=np.int64)
        names = [strings[c] for c in cands]
        starts, ends, best, gain = starts[order], starts[order] + span_len[order], best[order], gain[order]
        cost0 = cost[span_first[order] + order] if want_costs else None
        cost = cost[cands + np.repeat(order, counts) + 1] if want_costs else None
        # (most texts of a large corpus hold no span at all: they share ONE empty result, so that the call costs per span)
        found = [ratebatch.Rescored(starts[:0], ends[:0], first[:1] * 0, [], cost0[:0] if want_costs else None,
                                    cost[:0] if want_costs else None, best[:0], gain[:0])] * n
        for i in np.unique(span_text).tolist():
            a, b = int(cut[i]), int(cut[i + 1])
            ca, cb = int(first[a]), int(first[b])
            found[i] = ratebatch.Rescored(starts[a:b], ends[a:b], first[a:b + 1] - ca, names[ca:cb],
                                          cost0[a:b] if want_costs else None, cost[ca:cb] if want_costs else None,
                                          best[a:b], gain[a:b])
        return found

    def lexicon(self, words):
        '''A ratebatch.Lexicon of `words` -- an iterable of strings in priority order, the most frequent first --, normalised
        and encoded with this rater's mapping: what `lexicon_neighbours` and `correct_words` look suspect words up in.  Empty
        entries, entries of more than 64 characters, entries with a character outside the mapping and duplicates (the first is
        kept) are dropped and counted in `.dropped`.  Its device copy is made at the first look-up on an engine and kept.
        ValueError for a mapping of more than 4096 characters.'''
        assert self.status > 1
        return ratebatch.Lexicon(words, self.mapping[0], self.voc_size)

    def channel(self, records, unit_bits=8.0, min_count=2, min_rate=0.0):
        '''A ratebatch.Channel from a table of confusions: what `lexicon_neighbours` and `correct_words` weigh the way from a
        word to a lexicon entry with.  records is `confusions`' result or an iterable of (source, target, count, occ) -- what
        `keraslm-rate confusions --counts` prints --, the source being what the OCR reads for the target; the strings are
        normalised and encoded with this rater's mapping.  A record costs round(16 * min(-log2(count / occ), 255))
        sixteenths of a bit, a plain edit round(16 * unit_bits).  Dropped and counted in `.dropped`: records below min_count
        or min_rate, with an empty source, a source equal to the target, a character outside the mapping, a side of more than
        4 characters; duplicates (the least cost is kept) and, beyond 1024 rules, those of least count.  Its device copy is
        made at the first look-up on an engine and kept.  ValueError for unit_bits outside 1/16 .. 255.9.'''
        assert self.status > 1
        return ratebatch.Channel(records, self.mapping[0], self.voc_size, unit_bits=unit_bits, min_count=min_count,
                                 min_rate=min_rate)

    def _channel_request(self, method, channel, max_bits):
        max_bits = float(max_bits)
        if not 0.0 <= max_bits <= 255.9:
            raise ValueError("%s: max_bits in 0 .. 255.9 (got %r)" % (method, max_bits))
        if not isinstance(channel, ratebatch.Channel) or not channel.same_mapping(self.mapping[0]) or channel.voc_size != self.voc_size:
            raise ValueError("%s: the channel was not built by this rater's `channel`, or the mapping has changed since" % method)
        return int(round(ratebulk.CHANNEL_SCALE * max_bits))

    def _lexicon_request(self, method, lexicon, max_dist, per_word):
        max_dist, per_word = int(max_dist), int(per_word)
        if not (0 <= max_dist <= ratebulk.LEXICON_DIST_MAX and 1 <= per_word <= ratebulk.LEXICON_K_MAX):
            raise ValueError("%s: max_dist in 0 .. %d and per_word in 1 .. %d (got %d, %d)"
                             % (method, ratebulk.LEXICON_DIST_MAX, ratebulk.LEXICON_K_MAX, max_dist, per_word))
        if not isinstance(lexicon, ratebatch.Lexicon) or not lexicon.same_mapping(self.mapping[0]) or lexicon.voc_size != self.voc_size:
            raise ValueError("%s: the lexicon was not built by this rater's `lexicon`, or the mapping has changed since" % method)
        return max_dist, per_word

    def _lexicon_lookup(self, words, lexicon, blank, method, on_device, on_host):
        """The sequence `lexicon_neighbours`, `lexicon_splits` and `lexicon_chains` share: the words normalised, made unique
        and encoded, offsets and ids uploaded in ONE buffer, on_device(lm, chars_d, order_d, q_pool_d, q_off_d) called for
        the DEVICE tensors of the look-up ([Q] or [Q, ..] int32 each) -- on an engine without `method` (the tests' CPU double)
        on_host(pool, q_off) for the arrays of its statement --, these laid side by side as one int32 [Q, width] table,
        downloaded ONCE and spread back over the duplicates.  No words, or a lexicon without an entry: every row is `blank`
        and nothing is launched.  Returns the table in input order."""
        words = [windows.normalize(w) for w in words]
        slot = {}
        for w in words:
            slot.setdefault(w, len(slot))
        unique = list(slot)
        Q = len(unique)
        out = np.tile(np.asarray(blank, dtype=np.int32), (Q, 1))
        if Q and len(lexicon):
            pool = windows.encode("".join(unique), self.mapping[0]).astype(np.int32)
            q_off = np.concatenate([[0], np.cumsum([len(w) for w in unique])]).astype(np.int64)
            lm = self.model
            if hasattr(lm, method):
                torch = lm.torch
                chars_d, order_d = lexicon.on_device(lm)
                both = torch.from_numpy(np.concatenate([q_off.view(np.int32), pool])).to(lm.device)
                res = on_device(lm, chars_d, order_d, both[2 * (Q + 1):], both[:2 * (Q + 1)].view(torch.int64))
                out = _np(torch.cat([t.reshape(Q, -1) for t in res], dim=1))
            else:
                out = np.concatenate([a.reshape(Q, -1) for a in on_host(pool, q_off)], axis=1)
        rows = np.asarray([slot[w] for w in words], dtype=np.int64)
        return out[rows] if len(rows) else out[:0]

    def lexicon_neighbours(self, words, lexicon, max_dist=2, per_word=8, channel=None, max_bits=12.0):
        '''Which entries of the lexicon could these words have been?  Returns a ratebatch.Neighbours in input order: per word
        `exact` (its own index in `lexicon.words`, -1: not an entry), `found` (how many entries lie within 1 .. max_dist
        edits -- Levenshtein distance, unit costs) and the first `per_word` of them ordered by (distance, index), that is the
        nearest first and the more frequent among equally near ones, with their distances; -1 fills the unused places.

        The words are normalised, made unique on the host and encoded; there is one upload (offsets and ids in one buffer), one
        kernel call (`HipLM.lexicon_neighbours`: every (word, entry) pair of the length classes within max_dist on the device)
        and one download of 8 + 8 * per_word bytes per distinct word; the result is spread back over the duplicates.  A word of
        more than 64 characters (or of none) is a neighbour of nothing.  A character outside the mapping keeps id 0 here, and id
        0 is an ordinary id of the look-up: two different unmapped characters are equal, as in `rescore` -- but no entry holds
        one, so such a position always costs an edit.  No words, or a lexicon without an entry, give their result without a
        launch.  An engine without `lexicon_neighbours` (the tests' CPU double) runs ratebulk.lexicon_neighbours_host.
        ValueError for max_dist outside 0 .. 8, per_word outside 1 .. 16, a lexicon of another mapping.

        With a channel (`channel`) the search is the weighted one (`HipLM.lexicon_channel`, the statement
        ratebulk.lexicon_channel_host): the entries within max_cost = round(16 * max_bits) sixteenths of a bit, a plain edit
        at the channel's unit and every rule at its cost; max_dist is not used, `exact` is the entry identical to the word,
        `dist` holds sixteenths of a bit and `bits` their float value (None without a channel).  The rules are uploaded once
        per channel and engine.  ValueError for a channel of another mapping, or max_bits outside 0 .. 255.9.'''
        assert self.status > 1
        max_dist, K = self._lexicon_request("lexicon_neighbours", lexicon, max_dist, per_word)
        max_cost = None if channel is None else self._channel_request("lexicon_neighbours", channel, max_bits)
        V, lex = self.voc_size, (lexicon.chars, lexicon.order, lexicon.class_first)
        if channel is None:
            on_device = lambda lm, chars_d, order_d, q_pool_d, q_off_d: lm.lexicon_neighbours(
                chars_d, order_d, lexicon.class_first, V, q_pool_d, q_off_d, max_dist, K)
            on_host = lambda pool, q_off: ratebulk.lexicon_neighbours_host(pool, q_off, *lex, V, max_dist, K)
        else:
            on_device = lambda lm, chars_d, order_d, q_pool_d, q_off_d: lm.lexicon_channel(
                chars_d, order_d, lexicon.class_first, V, q_pool_d, q_off_d, *channel.on_device(lm), channel.unit, max_cost, K)
            on_host = lambda pool, q_off: ratebulk.lexicon_channel_host(pool, q_off, *lex, V, channel.rules, channel.cost,
                                                                        channel.unit, max_cost, K)
        # (exact, found, index [K], dist [K] per distinct word)
        out = self._lexicon_lookup(words, lexicon, [-1, 0] + [-1] * (2 * K), 'lexicon_neighbours' if channel is None else
                                   'lexicon_channel', on_device, on_host)
        dist = out[:, 2 + K:].copy()
        bits = None if channel is None else np.where(dist >= 0, dist / float(ratebulk.CHANNEL_SCALE), np.nan)
        return ratebatch.Neighbours(lexicon, out[:, 0].copy(), out[:, 1].copy(), out[:, 2:2 + K].copy(), dist, bits)

    def lexicon_splits(self, words, lexicon, max_dist=1, min_part=2, per_word=4):
        '''Where could these words be TWO entries of the lexicon run together (`ofthe`)?  Returns a ratebatch.Splits in input
        order: per word `found` (at how many places it falls into two entries, each half of at least `min_part` characters,
        within max_dist edits in all -- the lost delimiter is one of them, so max_dist=1 asks for two exact halves) and the
        first `per_word` places ordered by (distance, the larger of the two entries' indices, place), with the entries and the
        distance; -1 fills the unused places.  Per place and side only the nearest entry counts, the more frequent among
        equally near ones.

        As in `lexicon_neighbours` the words are normalised, made unique on the host and encoded; one upload, one kernel call
        (`HipLM.lexicon_splits`: no pairs of entries are formed, two walks over the shorter length classes give every place's
        nearest entry on either side), one download of 4 + 16 * per_word bytes per distinct word, spread back over the
        duplicates.  A word of more than 64 characters, or of fewer than 2 * min_part, has no such place.  No words, or a lexicon
        without an entry, give their result without a launch.  An engine without `lexicon_splits` (the tests' CPU double) runs
        ratebulk.lexicon_splits_host.  ValueError for max_dist outside 1 .. 8, min_part outside 1 .. 32, per_word outside
        1 .. 16, a lexicon of another mapping.'''
        assert self.status > 1
        max_dist, K = self._lexicon_request("lexicon_splits", lexicon, max_dist, per_word)
        min_part = int(min_part)
        if max_dist < 1 or not 1 <= min_part <= ratebulk.LEXICON_MIN_PART_MAX:
            raise ValueError("lexicon_splits: max_dist in 1 .. %d and min_part in 1 .. %d (got %d, %d)"
                             % (ratebulk.LEXICON_DIST_MAX, ratebulk.LEXICON_MIN_PART_MAX, max_dist, min_part))
        V, lex = self.voc_size, (lexicon.chars, lexicon.order, lexicon.class_first)
        # (found, at [K], left [K], right [K], dist [K] per distinct word)
        out = self._lexicon_lookup(
            words, lexicon, [0] + [-1] * (4 * K), 'lexicon_splits',
            lambda lm, chars_d, order_d, q_pool_d, q_off_d: lm.lexicon_splits(chars_d, order_d, lexicon.class_first, V, q_pool_d,
                                                                              q_off_d, max_dist, min_part, K),
            lambda pool, q_off: ratebulk.lexicon_splits_host(pool, q_off, *lex, V, max_dist, min_part, K))
        return ratebatch.Splits(lexicon, out[:, 0].copy(), *(out[:, 1 + f * K:1 + (f + 1) * K].copy() for f in range(4)))

    def _chain_links(self, method, links):
        """the linking elements of `lexicon_chains`, normalised, and their ids as int32 [n, 4] (len, ids[3])"""
        links = [windows.normalize(one) for one in ([links] if isinstance(links, str) else links)]
        if len(links) > ratebulk.LEXICON_LINKS_MAX:
            raise ValueError("%s: at most %d links (got %d)" % (method, ratebulk.LEXICON_LINKS_MAX, len(links)))
        for one in links:
            if not 1 <= len(one) <= ratebulk.LEXICON_LINK_LEN_MAX or any(not 0 < self.mapping[0].get(c, 0) < self.voc_size for c in one):
                raise ValueError("%s: a link is 1 .. %d mapped characters (got %r)" % (method, ratebulk.LEXICON_LINK_LEN_MAX, one))
        return links, ratebulk.lexicon_links_host([[self.mapping[0][c] for c in one] for one in links], self.voc_size)

    def lexicon_chains(self, words, lexicon, max_parts=4, min_part=2, links=(), per_word=None):
        '''Are these words CHAINS of entries of the lexicon -- compounds (`dampf|schiff|fahrt`), or words that lost more than
        one space (`inthehouse`)?  Returns a ratebatch.Chains in input order: per word and per number of parts p in
        1 .. max_parts whether it is p exact entries end to end, each of at least `min_part` characters, and one such chain --
        the one whose rarest piece is most frequent, ties as ratebulk.lexicon_chains_host settles them.  `links` are linking
        elements (`s`, `es`, `n`: strings of 1 .. 3 mapped characters, at most 8) that may stand between two pieces; they
        belong to no piece, do not count towards min_part and never stand at the word's ends.  per_word is not used (every p
        has its one row); it is there for the family's signature.

        As in `lexicon_neighbours` the words are normalised, made unique on the host and encoded; one upload, one kernel call
        (`HipLM.lexicon_chains`: one walk over the length classes min_part .. m matches every substring of the word, a small
        DP follows it), one download of 4 + 4 * P + 12 * P * P bytes per distinct word, spread back over the duplicates.  A
        word of more than 64 characters, or of fewer than min_part, is no chain.  No words, or a lexicon without an entry,
        give their result without a launch.  An engine without `lexicon_chains` (the tests' CPU double) runs
        ratebulk.lexicon_chains_host.  ValueError for max_parts outside 2 .. 8, min_part outside 1 .. 32, more than 8 links,
        a link of no or of more than 3 characters or with a character outside the mapping, a lexicon of another mapping.'''
        assert self.status > 1
        self._lexicon_request("lexicon_chains", lexicon, 0, 1)
        P, min_part = int(max_parts), int(min_part)
        if not (2 <= P <= ratebulk.LEXICON_PARTS_MAX and 1 <= min_part <= ratebulk.LEXICON_MIN_PART_MAX):
            raise ValueError("lexicon_chains: max_parts in 2 .. %d and min_part in 1 .. %d (got %d, %d)"
                             % (ratebulk.LEXICON_PARTS_MAX, ratebulk.LEXICON_MIN_PART_MAX, P, min_part))
        links, link_ids = self._chain_links("lexicon_chains", links)
        V, lex = self.voc_size, (lexicon.chars, lexicon.order, lexicon.class_first)
        # (found, worst [P], entry, start, link [P, P] per distinct word)
        out = self._lexicon_lookup(
            words, lexicon, [0] + [-1] * (P + 3 * P * P), 'lexicon_chains',
            lambda lm, chars_d, order_d, q_pool_d, q_off_d: lm.lexicon_chains(chars_d, order_d, lexicon.class_first, V, q_pool_d,
                                                                              q_off_d, link_ids, P, min_part),
            lambda pool, q_off: ratebulk.lexicon_chains_host(pool, q_off, *lex, V, link_ids, P, min_part))
        cube = lambda f: out[:, 1 + P + f * P * P:1 + P + (f + 1) * P * P].reshape(-1, P, P).copy()
        return ratebatch.Chains(lexicon, out[:, 0].copy(), out[:, 1:1 + P].copy(), cube(0), cube(1), cube(2), links)

    def correct_words(self, texts, lexicon, contexts=None, max_dist=2, per_word=8, known=False, delimiters=None, k=3,
                      max_prob=0.01, min_rank=1, min_suspects=1, min_bits_per_char=0.0, min_chars=1, left=64, ahead=8,
                      min_gain=1.0, streams=1024, precision="bf16", channel=None, max_bits=12.0, channel_weight=1.0,
                      boundaries=False, min_part=2, joiner=" ", compounds=0, links=(), max_parts=2):
        '''From texts to lexicon-backed corrections: `suspect_words` -> the suspect words' nearest lexicon entries ->
        `rescore`.  Returns (found, rescored, bits): `found` and `bits` are `suspect_words(texts, contexts, delimiters=..,
        k=.., max_prob=.., min_rank=.., min_suspects=.., min_bits_per_char=.., min_chars=.., streams=.., precision=..)`'s;
        all selected words of all texts go through ONE `lexicon_neighbours(words, lexicon, max_dist, per_word)`; a word that is
        an entry itself (`exact` >= 0) yields no candidates unless known=True -- a word of the lexicon is left alone by default
        --, every other word its neighbours in order; `rescored` is `rescore(texts, ratebatch.word_edits(found, texts, table),
        contexts, streams=.., left=.., ahead=.., min_gain=.., precision=..)` with `table` the dict word -> neighbour strings.
        The edits are built on the host from the downloaded neighbours (8 bytes per candidate).  State and precision afterwards
        are as after `rescore`.  ValueError for what these three raise.

        With a channel (`channel`) the candidates are `lexicon_neighbours(words, lexicon, per_word=.., channel=..,
        max_bits=..)`'s -- the entries that are cheap under the learned confusions, max_dist is not used -- and the channel's
        bits enter the choice beside the model's: `rescore(.., prior=..)` with channel_weight * bits per candidate
        (`ratebatch.word_edits` returns them beside the edits).  channel_weight = 0.0 lets the model alone choose among the
        channel's candidates.  ValueError also for channel_weight < 0 or not finite.

        With boundaries=True (and max_dist >= 1) lost and spurious delimiters are hypotheses too.  SPLITS: every looked-up word
        (one that is no entry, or any word with known=True) of fewer than 64 characters also goes through ONE
        `lexicon_splits(words, lexicon, max_dist, min_part, per_word)`, and its strings `left + joiner + right` follow the
        word's neighbours among its candidates (a string equal to an earlier candidate, or of more than 64 characters, is
        dropped).  MERGES: the `ratebatch.join_edits(found, texts, .., joiner)` of the pairs with at least one looked-up word go
        through ONE `lexicon_neighbours(joined, lexicon, max_dist - 1, per_word)`; here `exact` is a candidate and comes first,
        and every pair with candidates is an edit of its own over the two words and the joiner.  All edits go to the one
        `rescore`, ordered by text and start; overlapping spans are `Rescored.apply`'s business.  With a channel the merges are
        looked up through it at max_bits - unit_bits (none if that is negative) and cost their bits plus unit_bits for the
        joiner, a split costs unit_bits * dist, both times channel_weight.  ValueError also for min_part outside 1 .. 32 and for
        a joiner that is not one mapped character which the delimiter table holds.

        With compounds=P (2 .. 8) a word that is no entry but a CHAIN of 2 .. P entries, each of at least min_part characters
        and `links` allowed between them (`lexicon_chains`), counts as an entry: every looked-up word that is no entry goes
        through ONE `lexicon_chains(words, lexicon, P, min_part, links)`, and a chain yields no candidates unless known=True
        and is "not looked up" for the boundary hypotheses.  With boundaries=True and max_parts >= 3 (at most 8) more than one
        lost delimiter is a hypothesis: the words that go to `lexicon_splits` also go through ONE `lexicon_chains(words,
        lexicon, max_parts, min_part, links=())`, and its strings of 3 .. max_parts exact entries follow the splits' among the
        word's candidates (duplicates and strings of more than 64 characters dropped); with a channel each costs
        channel_weight * unit_bits * (p - 1).  At compounds=0 and max_parts=2, the defaults, `lexicon_chains` is not called.
        ValueError also for compounds other than 0 or 2 .. 8, max_parts outside 2 .. 8 and what `lexicon_chains` raises for
        the links.'''
        max_dist, per_word = self._lexicon_request("correct_words", lexicon, max_dist, per_word)
        boundaries = bool(boundaries) and max_dist >= 1
        if boundaries:
            min_part, joiner = int(min_part), windows.normalize(joiner)
            if not 1 <= min_part <= ratebulk.LEXICON_MIN_PART_MAX:
                raise ValueError("correct_words: min_part in 1 .. %d (got %d)" % (ratebulk.LEXICON_MIN_PART_MAX, min_part))
            delim = self._delimiter_table(delimiters)
            is_delimiter = lambda c: bool(0 < self.mapping[0].get(c, 0) < self.voc_size and delim[self.mapping[0][c]])
            if len(joiner) != 1 or not is_delimiter(joiner):
                raise ValueError("correct_words: joiner is one mapped character among the delimiters (got %r)" % (joiner,))
            max_parts = int(max_parts)
            if not 2 <= max_parts <= ratebulk.LEXICON_PARTS_MAX:
                raise ValueError("correct_words: max_parts in 2 .. %d (got %d)" % (ratebulk.LEXICON_PARTS_MAX, max_parts))
        compounds = int(compounds)
        if compounds:
            min_part = int(min_part)
            if not (2 <= compounds <= ratebulk.LEXICON_PARTS_MAX and 1 <= min_part <= ratebulk.LEXICON_MIN_PART_MAX):
                raise ValueError("correct_words: compounds 0 or in 2 .. %d, min_part in 1 .. %d (got %d, %d)"
                                 % (ratebulk.LEXICON_PARTS_MAX, ratebulk.LEXICON_MIN_PART_MAX, compounds, min_part))
            self._chain_links("correct_words", links)      # (their ValueErrors before any rating)
        channel_weight = float(channel_weight)
        if channel is not None:
            self._channel_request("correct_words", channel, max_bits)
            if not (np.isfinite(channel_weight) and channel_weight >= 0.0):
                raise ValueError("correct_words: channel_weight >= 0, finite (got %r)" % channel_weight)
        texts = list(texts)
        found, bits = self.suspect_words(texts, contexts, delimiters=delimiters, k=k, streams=streams, max_prob=max_prob,
                                         min_rank=min_rank, min_suspects=min_suspects, min_bits_per_char=min_bits_per_char,
                                         min_chars=min_chars, precision=precision)
        words = [w for one, text in zip(found, texts) for w in one.strings(windows.normalize(text))]
        near = self.lexicon_neighbours(words, lexicon, max_dist=max_dist, per_word=per_word, channel=channel, max_bits=max_bits)
        first = {}
        for i, word in enumerate(words):
            first.setdefault(word, i)
        # a word that is an entry is left alone -- and so is, with compounds, one that is a chain of 2 .. compounds entries
        as_entry = dict((word, bool(near.exact[i] >= 0)) for word, i in first.items())
        if compounds:
            unknown = [word for word in first if not as_entry[word]]
            chains = self.lexicon_chains(unknown, lexicon, compounds, min_part, links)
            for j, word in enumerate(unknown):
                as_entry[word] = bool(int(chains.found[j]) & ~1)
        table, weights = {}, {}
        for word, i in first.items():
            table[word] = near.strings(i) if known or not as_entry[word] else []
            if channel is not None:
                weights[word] = [channel_weight * float(b) for b in near.bits[i][:len(table[word])]]
        unit_bits = None if channel is None else channel.unit / float(ratebulk.CHANNEL_SCALE)
        if boundaries:
            looked = dict((word, bool(known or not as_entry[word])) for word in first)
            apart = [word for word in table if looked[word] and len(word) < ratebulk.SPAN_LEN_MAX]
            splits = self.lexicon_splits(apart, lexicon, max_dist=max_dist, min_part=min_part, per_word=per_word)
            for i, word in enumerate(apart):
                for string, dist in zip(splits.strings(i, joiner), splits.dist[i]):
                    if string not in table[word] and len(string) <= ratebulk.SPAN_LEN_MAX:
                        table[word].append(string)
                        if channel is not None:
                            weights[word].append(channel_weight * unit_bits * int(dist))
            if max_parts >= 3:
                # more than one lost delimiter: the word as 3 .. max_parts exact entries, behind the pairs
                longer = self.lexicon_chains(apart, lexicon, max_parts, min_part, links=())
                for i, word in enumerate(apart):
                    parts = [p for p in range(3, max_parts + 1) if (int(longer.found[i]) >> (p - 1)) & 1]
                    for string, p in zip(longer.strings(i, joiner, min_parts=3), parts):
                        if string not in table[word] and len(string) <= ratebulk.SPAN_LEN_MAX:
                            table[word].append(string)
                            if channel is not None:
                                weights[word].append(channel_weight * unit_bits * (p - 1))
        if channel is None:
            edits, prior = ratebatch.word_edits(found, texts, table), None
        else:
            edits, prior = ratebatch.word_edits(found, texts, table, priors=weights)
        merge_bits = max_bits if channel is None else float(max_bits) - unit_bits
        if boundaries and merge_bits >= 0.0:
            joins = ratebatch.join_edits(found, texts, is_delimiter, joiner, only=looked.get)
            whole = self.lexicon_neighbours([j[3] for j in joins], lexicon, max_dist=max_dist - 1, per_word=per_word,
                                            channel=channel, max_bits=merge_bits)
            merges, merge_prior = [], []
            for j, (i, start, end, _) in enumerate(joins):
                strings = ([lexicon.words[int(whole.exact[j])]] if whole.exact[j] >= 0 else []) + whole.strings(j)
                if strings:
                    merges.append((i, start, end, strings))
                    if channel is not None:
                        cost = ([0.0] if whole.exact[j] >= 0 else []) + [float(b) for b in whole.bits[j][:len(strings)]]
                        merge_prior.append([channel_weight * (b + unit_bits) for b in cost[:len(strings)]])
            # one list ordered by text and start (a word's own edit in front of the pair that begins with it)
            edits = edits + merges
            both = sorted(range(len(edits)), key=lambda e: edits[e][:3] + (e,))
            if channel is not None:
                prior = [(prior + merge_prior)[e] for e in both]
            edits = [edits[e] for e in both]
        rescored = self.rescore(texts, edits, contexts, streams=streams, left=left, ahead=ahead, min_gain=min_gain,
                                precision=precision, prior=prior)
        return found, rescored, bits

    def align(self, texts, others, max_dist=32, join=0):
        '''Where does each of `texts` differ from its second reading in `others` (one string per side and pair)?  Returns one
        ratebatch.Alignment per pair: `dist`, the Levenshtein distance (unit costs) if it is at most max_dist, -1 if the two are
        further apart -- not readings of the same text --, and `spans`, the differences as (a_start, a_end, b_start, b_end):
        maximal runs of substitutions, insertions and deletions of the canonical alignment (a diagonal step before a deletion
        before an insertion, walking back from the ends), two of them with at most `join` equal characters between them made
        one.  join=0 reports what is there.

        Both sides are NFC-normalised and positions are those of the normalised strings, as everywhere in `rescore`; the texts
        are compared as code points, so the result does not depend on the model's mapping.  On the HIP engine there is one
        upload per side (offsets and code points in one buffer), one kernel call (`HipLM.align_pairs`, max_len the longest text
        of the call), the used spans are compacted on the device, and dist, the span counts and the spans come back in one
        download.  No pairs give their result without a launch.  An engine without `align_pairs` (the tests' CPU double) runs
        ratebulk.align_pairs_host.  Needs a loaded engine, not a stateful rater.  ValueError for unequal numbers of texts, a
        text of more than 4096 characters, max_dist outside 1 .. 255, join < 0.'''
        assert self.status > 1
        texts, others = [windows.normalize(t) for t in texts], [windows.normalize(t) for t in others]
        max_dist, join = int(max_dist), int(join)
        if len(texts) != len(others):
            raise ValueError("align: one witness per text (got %d and %d)" % (len(texts), len(others)))
        if not 1 <= max_dist <= ratebulk.ALIGN_DIST_MAX or join < 0:
            raise ValueError("align: max_dist in 1 .. %d and join >= 0 (got %d, %d)" % (ratebulk.ALIGN_DIST_MAX, max_dist, join))
        P = len(texts)
        max_len = max([len(t) for t in texts + others] or [0])
        if max_len > ratebulk.ALIGN_LEN_MAX:
            raise ValueError("align: a text of %d characters; at most %d -- cut pages into lines or paragraphs"
                             % (max_len, ratebulk.ALIGN_LEN_MAX))
        if P == 0:
            return []
        sides = []
        for strings in (texts, others):
            off = np.concatenate([[0], np.cumsum([len(t) for t in strings])]).astype(np.int64)
            sides.append((np.frombuffer("".join(strings).encode("utf-32-le", "surrogatepass"), dtype=np.int32), off))
        lm = self.model
        if hasattr(lm, 'align_pairs'):
            torch = lm.torch
            args = []
            for pool, off in sides:
                both = torch.from_numpy(np.concatenate([off.view(np.int32), pool])).to(lm.device)
                args += [both[2 * (P + 1):], both[:2 * (P + 1)].view(torch.int64)]
            dist, n_spans, spans = lm.align_pairs(*args, max_len, max_dist, join)
            used = torch.arange(max_dist, device=lm.device)[None, :] < n_spans[:, None]
            out = _np(torch.cat([dist, n_spans, spans[used].reshape(-1)]))
            dist, n_spans, spans = out[:P], out[P:2 * P], out[2 * P:].reshape(-1, 4)
        else:
            dist, n_spans, spans = ratebulk.align_pairs_host(sides[0][0], sides[0][1], sides[1][0], sides[1][1], max_len, max_dist, join)
            spans = spans[np.arange(max_dist)[None, :] < n_spans[:, None]]
        first = np.concatenate([[0], np.cumsum(n_spans)])
        return [ratebatch.Alignment(dist[p], spans[first[p]:first[p + 1]].copy()) for p in range(P)]

    def merge_witnesses(self, texts, witnesses, contexts=None, max_dist=32, join=1, left=64, ahead=8, min_gain=1.0, streams=1024,
                        precision="bf16"):
        '''From a text and other readings of it to the readings the model prefers: `align` -> `ratebatch.witness_edits` ->
        `rescore`.  witnesses is one sequence of strings per text, possibly empty: what a second OCR engine (or several) read
        in the same line or page.  All pairs of all texts go through ONE `align(.., max_dist, join)`; the differing spans become
        `rescore`'s edits, the witnesses' readings of a span its candidates (`witness_edits`: spans at a text's first character,
        spans of more than 64 characters on a side and witnesses further than max_dist edits away yield none and are counted);
        `rescore(texts, edits, contexts, streams=.., left=.., ahead=.., min_gain=.., precision=..)` rates them.  Returns
        (alignments, rescored, skipped): per text the list of its witnesses' `Alignment`s, `rescore`'s result, and
        `witness_edits`' counts by reason.

        join defaults to 1 here and to 0 in `align`: two differences one character apart are ONE hypothesis to a model that
        reads `ahead` = 8 characters on -- rated apart, each would be held against a continuation that holds the other's
        error --, while `align` reports what is there.  State and precision afterwards are as after `rescore`.  ValueError for
        what `align` and `rescore` raise, and for a number of witness lists other than the number of texts.'''
        texts = list(texts)
        witnesses = [list(w) for w in witnesses]
        if len(witnesses) != len(texts):
            raise ValueError("merge_witnesses: one sequence of witnesses per text (got %d for %d texts)" % (len(witnesses), len(texts)))
        pairs = [(i, w) for i, readings in enumerate(witnesses) for w in range(len(readings))]
        flat = self.align([texts[i] for i, _ in pairs], [witnesses[i][w] for i, w in pairs], max_dist=max_dist, join=join)
        edits, skipped = ratebatch.witness_edits(flat, pairs, texts, witnesses)
        rescored = self.rescore(texts, edits, contexts, streams=streams, left=left, ahead=ahead, min_gain=min_gain, precision=precision)
        alignments = [[] for _ in texts]
        for one, (i, _) in zip(flat, pairs):
            alignments[i].append(one)
        return alignments, rescored, skipped

    def consensus(self, texts, witnesses, contexts=None, max_dist=32, join=1, vote_bits=0.0, left=64, ahead=8, min_gain=1.0,
                  streams=1024, precision="bf16", want_costs=True):
        '''`merge_witnesses` for texts with SEVERAL witnesses: the witnesses' differences are clustered across witnesses, so
        that differences which overlap -- or lie at most `join` equal characters apart -- are ONE hypothesis however many
        engines take part in it; every witness is read over the whole cluster, equal readings are one candidate, and how many
        witnesses give a reading counts.  witnesses is one sequence of strings per text, possibly empty, at most 64.  Returns
        (found, dists, skipped): `found` one ratebatch.Consensus per text (a `Rescored` with votes; the texts without a
        cluster share one empty result), dists[i] int32, the distance of every witness of text i as `align` gives it, and
        `skipped`, what yielded no hypothesis, by reason: "different" -- witnesses further than max_dist edits away --,
        "first" -- clusters at a text's first character --, "long" -- clusters with more than 64 characters as written or in a
        reading.  The definitions are ratebulk.witness_clusters_host's.

        A reading's score is its cost in bits as `rescore` defines it, minus vote_bits per vote -- the text as written has its
        own vote and that of every witness that agrees with it over the cluster --; `best`, `gain` and min_gain are
        `rescore`'s over the scores, and cost0 and cost hold the scores.  vote_bits = 0.0 is the model alone: with one witness
        per text the result is `merge_witnesses`' `rescored`.

        On the HIP engine: one upload per side as in `align`, the corpus as in `rescore`, the witnesses' ids; `align_pairs`
        and `witness_clusters` are chained with nothing read between them, then the 64 bytes of the clusters' counts are read
        -- the only wait before rating -- and the S + 1 candidate offsets for the chunks; `witness_pool`, `rescore`'s chunk
        loop on the arrays as they lie on the device, the votes subtracted there, one `span_pick`; one download of what the
        results hold.  No `Alignment` is made and no span passes through Python.  No pairs or no clusters give their result
        without a rating launch.  An engine without `witness_clusters` (the tests' CPU double) runs the numpy statements.
        State and precision afterwards are as after `rescore`.  ValueError for what `align` and `rescore` raise, vote_bits
        < 0, a number of witness lists other than the number of texts, more than 64 witnesses of a text.'''
        texts, contexts = self._rating_request("consensus", texts, contexts, precision)[:2]
        if not self.stateful:
            raise ValueError('consensus needs a stateful rater: it rates through stateful windows')
        texts = [windows.normalize(t) for t in texts]
        witnesses = [[windows.normalize(w) for w in readings] for readings in witnesses]
        n = len(texts)
        if len(witnesses) != n:
            raise ValueError("consensus: one sequence of witnesses per text (got %d for %d texts)" % (len(witnesses), n))
        max_dist, join, vote_bits = int(max_dist), int(join), float(vote_bits)
        left, ahead, streams = int(left), int(ahead), max(1, int(streams))
        if not 1 <= max_dist <= ratebulk.ALIGN_DIST_MAX or join < 0:
            raise ValueError("consensus: max_dist in 1 .. %d and join >= 0 (got %d, %d)" % (ratebulk.ALIGN_DIST_MAX, max_dist, join))
        if not vote_bits >= 0.0:
            raise ValueError("consensus: vote_bits >= 0 (got %r)" % vote_bits)
        if left < 1 or ahead < 0:
            raise ValueError("left >= 1 and ahead >= 0 (got %d, %d)" % (left, ahead))
        if left + ahead > 1024:
            raise ValueError("left + ahead <= 1024 (got %d, %d)" % (left, ahead))
        count = np.asarray([len(readings) for readings in witnesses], dtype=np.int64).reshape(n)
        if n and count.max() > ratebulk.WITNESS_MAX:
            raise ValueError("consensus: %d witnesses of a text; at most %d" % (count.max(), ratebulk.WITNESS_MAX))
        others = [w for readings in witnesses for w in readings]
        max_len = max([len(t) for t in texts + others] or [0])
        if max_len > ratebulk.ALIGN_LEN_MAX:
            raise ValueError("consensus: a text of %d characters; at most %d -- cut pages into lines or paragraphs"
                             % (max_len, ratebulk.ALIGN_LEN_MAX))
        P = len(others)
        pair_first = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
        offsets = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.int64)
        real = lambda m: np.zeros(m, dtype=np.float64) if want_costs else None
        none = ratebatch.Consensus(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(1, dtype=np.int64), [], real(0),
                                   real(0), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float64), np.zeros(0, dtype=np.int32),
                                   np.zeros(0, dtype=np.int32))
        found = [none] * n
        if P == 0:
            return found, [np.zeros(0, dtype=np.int32)] * n, dict(different=0, first=0, long=0)
        lm = self.model
        if precision == "split":
            self._ensure_precision()
        sides = []
        for strings in ([t for t, c in zip(texts, count.tolist()) for _ in range(c)], others):
            off = np.concatenate([[0], np.cumsum([len(t) for t in strings])]).astype(np.int64)
            sides.append((np.frombuffer("".join(strings).encode("utf-32-le", "surrogatepass"), dtype=np.int32), off))
        joined = "".join(others)
        corpus = self._corpus_ids("".join(texts), offsets)
        b_ids = windows.encode(joined, self.mapping[0]).astype(np.int32)
        clamped = {}      # (one context list for all texts is one object n times)
        for c in contexts:
            if id(c) not in clamped:
                clamped[id(c)] = windows.clamp_context(c)
        text_ctx = np.asarray([clamped[id(c)] for c in contexts], dtype=np.int32).reshape(n, -1)
        device = hasattr(lm, 'witness_clusters')
        if device:
            torch = lm.torch
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(lm.device)
            args = []
            for pool, off in sides:
                both = torch.from_numpy(np.concatenate([off.view(np.int32), pool])).to(lm.device)
                args += [both[2 * (P + 1):], both[:2 * (P + 1)].view(torch.int64)]
            both = up(np.concatenate([pair_first, offsets]))
            source = [up(corpus), both[n + 1:], up(text_ctx) if lm.n_ctx else None]
            b_ids_d = up(b_ids)
            aligned = lm.align_pairs(*args, max_len, max_dist, join)
            out = lm.witness_clusters(args[2], args[3], *aligned, both[:n + 1], both[n + 1:], join)
            stats = _np(out[7])      # (64 bytes: the only wait before rating)
        else:
            source = [corpus, offsets, text_ctx]
            aligned = ratebulk.align_pairs_host(sides[0][0], sides[0][1], sides[1][0], sides[1][1], max_len, max_dist, join)
            out = ratebulk.witness_clusters_host(sides[1][0], sides[1][1], *aligned, pair_first, offsets, join)
            stats = out[7]
        S, C, n_pool, M = (int(v) for v in stats[:4])
        assert stats[7] == 0
        skipped = dict(different=int(stats[4]), first=int(stats[5]), long=int(stats[6]))
        cut_dists = lambda dist: [dist[a:b] for a, b in zip(pair_first[:-1].tolist(), pair_first[1:].tolist())]
        if S == 0:
            return found, cut_dists(_np(aligned[0]).astype(np.int32)), skipped
        M = max(M, 1)
        if left + ahead + M - 1 > 1024:
            raise ValueError("left + ahead + %d - 1 <= 1024 (got %d, %d)" % (M, left, ahead))
        T = max(left + ahead + M - 1, ratebulk.MIN_T)
        span_first = _np(out[3][:S + 1])
        chunks = ratebulk.span_chunks(span_first, streams)
        pool = (lm.witness_pool if device else ratebulk.witness_pool_host)(b_ids_d if device else b_ids, out[4], out[5], C, n_pool)
        spans = [out[0][:S], out[1][:S], out[2][:S], out[3][:S + 1], pool, out[5][:C + 1]]
        cost, valid = self._span_row_costs(source, spans, chunks, precision, left, ahead, M, T)
        votes = out[6][:S + C]
        if device:
            if vote_bits:
                cost = cost - votes.to(torch.float64) * vote_bits
            best, gain, cost = lm.span_pick(cost, valid, spans[3], float(min_gain), want_costs=want_costs)
            lm.rate_status_check()
            whole = _np(torch.cat([aligned[0].to(torch.int64), spans[0].to(torch.int64), spans[1], spans[2].to(torch.int64),
                                   out[4][:C], spans[5], votes.to(torch.int64), best.to(torch.int64)]))
            parts = np.split(whole, np.cumsum([P, S, S, S, C, C + 1, S + C]))
            dist, span_text, span_start, span_len, cand_src, cand_off, votes, best = parts
            best, gain, cost = best.astype(np.int32), _np(gain), _np(cost) if want_costs else None
        else:
            if vote_bits:
                cost = cost - votes.astype(np.float64) * vote_bits
            best, gain, cost = ratebulk.span_pick_host(cost, valid, span_first, float(min_gain))
            cost = cost if want_costs else None
            dist, span_text, span_start, span_len, cand_src, cand_off = aligned[0], out[0][:S], out[1][:S], out[2][:S], out[4][:C], spans[5]
        lm.reset_states(1)
        # per text: its clusters lie together and ascend -- everything gathered once, then cut
        span_text = span_text.astype(np.int64)
        starts = span_start.astype(np.int64) - offsets[span_text]
        ends = starts + span_len
        sizes = cand_off[1:] - cand_off[:-1]
        names = [joined[a:a + m] for a, m in zip(cand_src.tolist(), sizes.tolist())]
        written = span_first[:S] + np.arange(S, dtype=np.int64)
        rows = np.arange(C, dtype=np.int64) + np.repeat(np.arange(S, dtype=np.int64), span_first[1:] - span_first[:-1]) + 1
        votes = votes.astype(np.int32)
        cut = np.searchsorted(span_text, np.arange(n + 1), side="left")
        for i in np.unique(span_text).tolist():
            a, b = int(cut[i]), int(cut[i + 1])
            ca, cb = int(span_first[a]), int(span_first[b])
            found[i] = ratebatch.Consensus(starts[a:b], ends[a:b], span_first[a:b + 1] - ca, names[ca:cb],
                                           cost[written[a:b]] if want_costs else None, cost[rows[ca:cb]] if want_costs else None,
                                           best[a:b], gain[a:b], votes[written[a:b]], votes[rows[ca:cb]])
        return found, cut_dists(dist.astype(np.int32)), skipped

    def _corpus_ids(self, joined, offsets):
        '''the ids of all texts of a call, encoded in one go (`joined` their concatenation, offsets [n + 1]); a character
        outside the mapping is reported with its position in its text, as `rate` does, and keeps id 0'''
        corpus = windows.encode(joined, self.mapping[0]).astype(np.int32)
        for g in np.nonzero(corpus == 0)[0]:
            if joined[int(g)] not in self.mapping[0]:
                self._unmapped_input(joined[int(g)], int(g - offsets[np.searchsorted(offsets, g, side="right") - 1]))
        return corpus

    _CONFUSION_ROOM = 65536      # rows of the first `confusion_counts` call of `confusions`

    def confusions(self, texts, truths, max_dist=32, join=0, max_chars=4):
        '''The table of OCR confusions that `texts` (OCR output) amount to when held against `truths` (ground truth of the
        same lines or pages, one string per side and pair): which strings were read as which, how often, and how often each
        source stands in the OCR texts at all.  Returns a ratebatch.Confusions; its `rules()` is what `confusion_edits` and
        `keraslm-rate rescore --confusions` take.

        A record is a differing span of `align(texts, truths, max_dist, join)` -- the OCR's side the source, the truth's the
        target, "" for characters the OCR added --; where the OCR LOST characters the span is anchored on the character in
        front (at a text's beginning: behind), so that every rule has a source.  Spans with more than max_chars characters on
        a side after anchoring, spans of an empty text and pairs further than max_dist edits apart are counted in `skipped`.

        Both sides are normalised and encoded as in `align`: one upload per side.  On the HIP engine `align_pairs` and
        `confusion_counts` are chained with no download between them, with room for 65536 records -- once more with room for
        all if there are more: the number of records is read first, eight bytes and the only wait --, and dist, the counts and
        the R records come back in one transfer.  No pairs give an empty
        table without a launch.  An engine without `confusion_counts` (the tests' CPU double) runs the numpy statements.
        ValueError for what `align` raises and for max_chars outside 1 .. 4.'''
        assert self.status > 1
        texts, truths = [windows.normalize(t) for t in texts], [windows.normalize(t) for t in truths]
        max_dist, join, max_chars = int(max_dist), int(join), int(max_chars)
        if len(texts) != len(truths):
            raise ValueError("confusions: one truth per text (got %d and %d)" % (len(texts), len(truths)))
        if not 1 <= max_dist <= ratebulk.ALIGN_DIST_MAX or join < 0:
            raise ValueError("confusions: max_dist in 1 .. %d and join >= 0 (got %d, %d)" % (ratebulk.ALIGN_DIST_MAX, max_dist, join))
        if not 1 <= max_chars <= ratebulk.CONFUSION_CHARS_MAX:
            raise ValueError("confusions: max_chars in 1 .. %d (got %d)" % (ratebulk.CONFUSION_CHARS_MAX, max_chars))
        P = len(texts)
        max_len = max([len(t) for t in texts + truths] or [0])
        if max_len > ratebulk.ALIGN_LEN_MAX:
            raise ValueError("confusions: a text of %d characters; at most %d -- cut pages into lines or paragraphs"
                             % (max_len, ratebulk.ALIGN_LEN_MAX))
        if P == 0:
            return ratebatch.Confusions(np.full((0, 10), -1, dtype=np.int32), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64),
                                        np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int64))
        sides = []
        for strings in (texts, truths):
            off = np.concatenate([[0], np.cumsum([len(t) for t in strings])]).astype(np.int64)
            sides.append((np.frombuffer("".join(strings).encode("utf-32-le", "surrogatepass"), dtype=np.int32), off))
        lm = self.model
        if hasattr(lm, 'confusion_counts'):
            torch = lm.torch
            args = []
            for pool, off in sides:
                both = torch.from_numpy(np.concatenate([off.view(np.int32), pool])).to(lm.device)
                args += [both[2 * (P + 1):], both[:2 * (P + 1)].view(torch.int64)]
            aligned = lm.align_pairs(*args, max_len, max_dist, join)
            room = self._CONFUSION_ROOM
            rules, count, occ, stats = lm.confusion_counts(*args, *aligned, max_chars, room)
            R = int(stats[0].item())
            if R > room:
                rules, count, occ, stats = lm.confusion_counts(*args, *aligned, max_chars, R)
            out = _np(torch.cat([aligned[0].to(torch.int64), stats, count[:R], occ[:R], rules[:R].reshape(-1).to(torch.int64)]))
            dist, stats, count, occ = out[:P].astype(np.int32), out[P:P + 4], out[P + 4:P + 4 + R], out[P + 4 + R:P + 4 + 2 * R]
            rules = out[P + 4 + 2 * R:].astype(np.int32).reshape(R, 10)
        else:
            aligned = ratebulk.align_pairs_host(sides[0][0], sides[0][1], sides[1][0], sides[1][1], max_len, max_dist, join)
            dist = aligned[0]
            rules, count, occ, stats = ratebulk.confusion_counts_host(sides[0][0], sides[0][1], sides[1][0], sides[1][1], *aligned,
                                                                      max_chars, self._CONFUSION_ROOM)
            if stats[0] > self._CONFUSION_ROOM:
                rules, count, occ, stats = ratebulk.confusion_counts_host(sides[0][0], sides[0][1], sides[1][0], sides[1][1], *aligned,
                                                                          max_chars, int(stats[0]))
            R = int(stats[0])
            rules, count, occ = rules[:R], count[:R], occ[:R]
        return ratebatch.Confusions(rules, count, occ, stats, dist, np.array([len(t) for t in truths], dtype=np.int64))

    def _contexts_per_text(self, contexts, n):
        '''None, one context list for all texts, or one per text -> one list per text (as `rate_batch` reads them)'''
        if contexts is None or len(contexts) == 0:
            return [self.underspecify_contexts()] * n
        if isinstance(contexts[0], (int, np.integer)):
            return [list(contexts)] * n
        assert len(contexts) == n, "one context list per text"
        return [list(c) if (c is not None and len(c)) else self.underspecify_contexts() for c in contexts]

    def rate2(self, text, context=None):
        '''Rate a string one by one (rating.py:531-576): resets the state, feeds one
        character per step, returns [(char, prob)] and the perplexity 2^(H/len).'''
        assert self.status > 1
        assert self.incremental is False
        if not context:
            context = self.underspecify_contexts()
        context = windows.clamp_context(context)
        self._ensure_precision()
        text = windows.normalize(text)
        lm = self.model
        if not self.stateful:
            return self._rate2_stateless(text, context)
        lm.reset_states(1)
        z = np.asarray(context, dtype=np.int32).reshape(1, 1, -1)
        entropy = 0
        result = []
        prev = 0
        for i, char in enumerate(text):
            if char not in self.mapping[0]:
                self.logger.error('unmapped character "%s" at input position %d', char, i)
                idx = 0
            else:
                idx = self.mapping[0][char]
            if i == 0:
                result.append((char, 1.0))
            else:
                pred = _np(lm.forward_window(np.array([[prev]], dtype=np.int32), z))[0, 0]
                prob = float(pred[idx])
                entropy -= log(max(prob, 1e-99), 2)
                result.append((char, prob))
            prev = idx
        return result, pow(2.0, entropy / len(text))

    def _rate2_stateless(self, text, context):
        '''rating.py:548-576 for stateful=False: a window that slides by one character per step, filled from
        the right; evaluated over its last i columns (variable length) or whole, left zeros included'''
        lm = self.model
        L, n_ctx = self.length, len(context)
        x = np.zeros((1, L), dtype=np.int32)
        z = np.zeros((1, L, n_ctx), dtype=np.int32)
        entropy = 0
        result = []
        for i, char in enumerate(text):
            if char not in self.mapping[0]:
                self.logger.error('unmapped character "%s" at input position %d', char, i)
                idx = 0
            else:
                idx = self.mapping[0][char]
            if i == 0:
                result.append((char, 1.0))
            else:
                xi, zi = (x[:, -i:], z[:, -i:]) if self.variable_length else (x, z)
                lm.reset_states(1)
                pred = _np(lm.forward_window(np.ascontiguousarray(xi), np.ascontiguousarray(zi)))[0, -1]
                prob = float(pred[idx])
                entropy -= log(max(prob, 1e-99), 2)
                result.append((char, prob))
            x = np.roll(x, -1, axis=1)
            z = np.roll(z, -1, axis=1)
            x[0, -1] = idx
            z[0, -1] = np.asarray(context, dtype=np.int32)
        return result, pow(2.0, entropy / len(text))

    rate_once = rate2   # historic name of the one-by-one rater (north_star / BASELINE.json)

    # ------------------------------------------------------------------ incremental step
    def _state_pool(self):
        if self._pool is None:
            self._pool = StatePool(self.model, self.depth)
        return self._pool

    def _ids(self, candidates):
        c_i = self.mapping[0]
        return np.fromiter((c_i.get(c, 0) for c in candidates), dtype=np.int32, count=len(candidates))

    def _predict_refs(self, candidates, states, context, heads=False, targets=None):
        """device-resident variant of predict(): states are StateRef (or None = zero
        state); returns (probs [n,V] float32 array, list of new StateRef).  All index vectors travel to
        the GPU in ONE transfer; with `heads` the first `depth` vectors of every new state come back with
        the probabilities, so that history clustering (rating.py:887-916) compares them on the host
        instead of synchronising with the GPU once per candidate pair.

        An engine with `step_host` (HipLM: kl_step_batch_host) takes the index vectors as host arrays inside its launches
        and delivers into host memory without a stream synchronisation; with `targets` (the character ids a lattice
        decoder will look at, rating.py:838-843) it returns probs [n] -- those probabilities alone."""
        pool = self._state_pool()
        n = len(candidates)
        ctx = np.asarray(windows.clamp_context(context), dtype=np.int32)
        lm = self.model
        if hasattr(lm, "step_host"):
            new, slots = pool.refs(n)
            zero = pool.zero_slot
            c_i = self.mapping[0]
            packed = np.array([[c_i.get(c, 0) for c in candidates], [s.slot if s is not None else zero for s in states], slots],
                              dtype=np.int32)
            key = (n, tuple(ctx.tolist()))
            if self._ctx_rows is None or self._ctx_rows[0] != key:      # (one context per page: the same rows edge after edge)
                self._ctx_rows = (key, np.tile(ctx, (n, 1)))
            probs, hv = lm.step_host(packed[0], self._ctx_rows[1], packed[1], packed[2],
                                     target=targets, head_k=self.depth if heads else 0)
            if heads:
                for r, v in zip(new, hv):
                    r.head = v
            return probs, new
        new = [pool.ref() for _ in range(n)]
        packed = np.empty((3 + len(ctx), n), dtype=np.int32)
        packed[0] = self._ids(candidates)
        packed[1] = np.fromiter((s.slot if s is not None else pool.zero_slot for s in states), dtype=np.int32, count=n)
        packed[2] = np.fromiter((r.slot for r in new), dtype=np.int32, count=n)
        packed[3:] = ctx[:, None]
        hv = None
        if hasattr(lm, "to_device_i32"):
            dev = lm.to_device_i32(packed)
            ctx_d = dev[3] if len(ctx) == 1 else dev[3:].t().contiguous()
            if heads and hasattr(lm, "step_slots_heads"):
                probs, hv = lm.step_slots_heads(dev[0], ctx_d, dev[1], dev[2], self.depth)      # (one copy to the host for both)
            else:
                probs = _np(lm.step_slots(dev[0], ctx_d, dev[1], dev[2]))
        else:
            probs = _np(lm.step_slots(packed[0], packed[3:].T.copy(), packed[1], packed[2]))
        if heads:
            if hv is None:
                hv = _np(lm.pool_heads(packed[2], self.depth))
            for r, v in zip(new, hv):
                r.head = v
        return probs, new

    def predict(self, candidates, initial_states, context=None):
        '''Predict character probabilities for n hypotheses at once, passing initial
        and final states explicitly (rating.py:578-639).  `initial_states[i]` is None
        (zero state), a list [h1,c1,...,hL,cL] of arrays, or a StateRef.  Returns
        (list of n probability arrays [V], list of n state lists of (1,W) arrays).'''
        assert self.status > 1
        assert self.stateful is False
        assert self.incremental is True
        assert len(candidates) == len(initial_states), \
            "number of inputs (%d) and number of states (%d) inconsistent" % (len(candidates), len(initial_states))
        if not context:
            context = self.underspecify_contexts()
        self._ensure_precision()
        pool = self._state_pool()
        n = len(candidates)
        refs, upload_slots, upload_vals = [], [], []
        for state in initial_states:
            if state is None or (not isinstance(state, StateRef) and not state):
                refs.append(None)
            elif isinstance(state, StateRef):
                refs.append(state)
            else:
                ref = pool.ref()
                upload_slots.append(ref.slot)
                upload_vals.append(np.stack([np.asarray(s, dtype=np.float32).reshape(self.width) for s in state]))
                refs.append(ref)
        if upload_slots:
            self.model.pool_write(upload_slots, np.stack(upload_vals))
        probs, new = self._predict_refs(candidates, refs, context)
        states = self.model.pool_read([r.slot for r in new])      # [n][2L][W]
        preds = [probs[i, :] for i in range(n)]
        final_states = [[states[i, k][None, :] for k in range(2 * self.depth)] for i in range(n)]
        return preds, final_states

    # ------------------------------------------------------------------ beam searches
    def generate(self, prefix, length, context=None, variants=1, device_beam=None):
        '''Generate `length` characters after `prefix` by beam search over the 10 best
        continuations with p >= 0.004 per hypothesis, 256 hypotheses wide
        (rating.py:642-709).  Returns `variants` strings, each starting with prefix[-1].

        device_beam (None: the attribute `self.device_beam`, which KERASLM_DEVICE_BEAM=1 turns on): on an engine with
        `beam_expand` the continuations are chosen and pruned where the probabilities are (kl_beam_expand), all `length`
        steps are enqueued without a wait and the strings are spelled from one log of back-pointers (genbeam.py).  Same
        strings; among exactly equal probabilities of one row the smaller id counts as the more probable.
        The costs of the returned strings are left in `self.generate_costs`.'''
        assert self.status > 1
        assert self.stateful is False
        assert self.incremental is True
        if not context:
            context = self.underspecify_contexts()
        self._ensure_precision()
        if device_beam is None:
            device_beam = self.device_beam
        if device_beam and hasattr(self.model, "beam_expand"):
            return self._generate_device(prefix, length, context, variants)
        state = None
        for char in prefix[:-1]:
            _, states = self._predict_refs([char], [state], context)
            state = states[0]
        next_fringe = [Node(state=state, value=prefix[-1], cost=0.0)]
        i_c = self.mapping[1]
        for _ in range(length):
            fringe = next_fringe
            preds, states = self._predict_refs([n.value for n in fringe], [n.state for n in fringe], context)
            # The reference insorts every continuation into one list ordered by cost and keeps the first
            # 256 (rating.py:699-707).  Same result, less Python: the order is kept on a parallel list of
            # float keys (insort_left = bisect_left, ties go in front), and a continuation that is
            # strictly worse than the current 256th can never return into the kept part, so it is
            # not even built.
            next_fringe, keys = [], []
            for j, n in enumerate(fringe):
                pred = preds[j]
                pred_best = np.argsort(pred)[-10:]
                pred_best = pred_best[np.searchsorted(pred[pred_best], 0.004):]
                costs = -np.log(pred[pred_best])
                state = states[j]
                base = n.cum_cost
                for best, cost in zip(pred_best, costs):
                    if best not in i_c:
                        continue
                    if len(keys) >= 256 and base + cost > keys[-1]:
                        continue
                    node = Node(parent=n, state=state, value=i_c[best], cost=cost)
                    pos = bisect_left(keys, node.cum_cost)
                    keys.insert(pos, node.cum_cost)
                    next_fringe.insert(pos, node)
                    if len(keys) > 256:
                        keys.pop()
                        next_fringe.pop()
        best = next_fringe[0:variants]
        self.generate_costs = [float(n.cum_cost) for n in best]
        return [''.join([n.value for n in res.to_sequence()]) for res in best]

    def _generate_device(self, prefix, length, context, variants, rows=256, fan=10):
        '''generate's search on the device (HipLM.beam_generate): the prefix warmed up in one engine call, 2 * rows working
        slots taken from the pool for the duration (and the pool grown) before anything is enqueued, one wait at the end.'''
        if length == 0:
            self.generate_costs = [0.0]
            return [prefix[-1]]
        pool = self._state_pool()
        lm = self.model
        c_i, i_c = self.mapping
        ctx = np.asarray(windows.clamp_context(context), dtype=np.int32)
        warm_ids = [c_i.get(c, 0) for c in prefix[:-1]]
        walk = getattr(lm, "walk_host", None)
        slots = pool.take_slots(2 * rows + (len(warm_ids) if walk else 0))
        try:
            slot0, state = pool.zero_slot, None
            if warm_ids and walk:
                warm = slots[2 * rows:]
                for at in range(0, len(warm_ids), 1024):      # (a walk's row takes up to 1024 steps)
                    part = warm_ids[at:at + 1024]
                    walk([len(part)], part, [0] * len(part), ctx[None, :], [slot0], warm[at:at + len(part)])
                    slot0 = warm[at + len(part) - 1]
            else:
                for char in prefix[:-1]:
                    _, states = self._predict_refs([char], [state], context)
                    state = states[0]
                if state is not None:
                    slot0 = state.slot
            valid = np.zeros(self.voc_size, dtype=np.uint8)
            valid[[i for i in i_c if 0 <= i < self.voc_size]] = 1
            log = lm.beam_generate(c_i.get(prefix[-1], 0), slot0, ctx, length, rows, fan, np.float32(0.004), valid,
                                   slots[:rows], slots[rows:2 * rows], pool.zero_slot)
        finally:
            pool.release_slots(slots)
        out = genbeam.backtrack(log, variants, i_c, prefix[-1])
        self.generate_costs = [float(c) for c in log[2][-1][:len(out)]]
        return out

    # ------------------------------------------------------------------ sampling
    def sample(self, prefix, length, context=None, variants=1, temperature=1.0, top_k=0, floor=0.0, seed=0):
        '''Draw `variants` continuations of `length` characters after `prefix` from the model's distribution: independent
        chains, each character drawn from the probabilities its own chain produced (`generate` returns the cheapest strings
        of a beam search instead).  Returns `variants` strings of 1 + length characters, each starting with prefix[-1]; their
        model costs (the sum of -log p along the string) are left in `self.sample_costs`.

        temperature: 1 draws from the distribution itself, below 1 sharpens it, 0 always takes the most probable character;
        top_k > 0 (up to 64): only the top_k most probable characters can be drawn; floor: nor characters with p < floor
        (the most probable one always can).  Only mapped characters are drawn.  The numbers come from a counter-based
        generator (Philox4x32-10) keyed by `seed` and counted by (position, chain): the same seed gives the same strings,
        and chain i does not depend on how many chains are drawn.  The rules in full: gensample.py, include/keraslm_hip.h (kl_sample_pick).

        On an engine with `sample_pick` (HipLM) the characters are drawn where the probabilities are, all `length` steps of up
        to 1024 chains enqueued without a wait (HipLM.sample_generate); more chains run in groups of 1024 that continue the row
        numbers.  Other engines step through `_predict_refs` and draw with gensample.pick_host.'''
        assert self.status > 1
        assert self.stateful is False
        assert self.incremental is True
        variants, length = int(variants), int(length)
        if variants < 1 or length < 0 or not prefix:
            raise ValueError("sample: a prefix, a length >= 0 and at least one variant, please")
        gensample.check_args(temperature, top_k, floor)
        if not context:
            context = self.underspecify_contexts()
        self._ensure_precision()
        self.sample_log = []
        if length == 0:
            self.sample_costs = [0.0] * variants
            return [prefix[-1]] * variants
        c_i, i_c = self.mapping
        valid = np.zeros(self.voc_size, dtype=np.uint8)
        valid[[i for i in i_c if 0 <= i < self.voc_size]] = 1
        args = (float(temperature), int(top_k), float(floor), int(seed))
        if hasattr(self.model, "sample_pick"):
            logs = self._sample_device(prefix, length, context, variants, valid, args)
        else:
            logs = self._sample_host(prefix, length, context, variants, valid, args)
        self.sample_log = logs
        self.sample_costs = [float(c) for log in logs for c in log[1][-1]]
        return [text for log in logs for text in gensample.spell(log, i_c, prefix[-1])]

    def _sample_device(self, prefix, length, context, variants, valid, args):
        '''sample's chains on the device: the prefix warmed up in one engine call (as _generate_device does), 2 * rows
        working slots (rows = the chains of a group, at most 1024) taken from the pool for the duration, one wait per group'''
        pool = self._state_pool()
        lm = self.model
        c_i = self.mapping[0]
        ctx = np.asarray(windows.clamp_context(context), dtype=np.int32)
        warm_ids = [c_i.get(c, 0) for c in prefix[:-1]]
        walk = getattr(lm, "walk_host", None)
        rows = min(variants, gensample.MAX_ROWS)
        slots = pool.take_slots(2 * rows + (len(warm_ids) if walk else 0))
        try:
            slot0, state = pool.zero_slot, None
            if warm_ids and walk:
                warm = slots[2 * rows:]
                for at in range(0, len(warm_ids), 1024):      # (a walk's row takes up to 1024 steps)
                    part = warm_ids[at:at + 1024]
                    walk([len(part)], part, [0] * len(part), ctx[None, :], [slot0], warm[at:at + len(part)])
                    slot0 = warm[at + len(part) - 1]
            else:
                for char in prefix[:-1]:
                    _, states = self._predict_refs([char], [state], context)
                    state = states[0]
                if state is not None:
                    slot0 = state.slot
            logs = []
            for row0 in range(0, variants, rows):
                n = min(rows, variants - row0)
                logs.append(lm.sample_generate(c_i.get(prefix[-1], 0), slot0, ctx, length, n, *args, valid, slots[:n],
                                               slots[rows:rows + n], pool.zero_slot,
                                               keep_probs=self.sample_keep_probs, row0=row0))
        finally:
            pool.release_slots(slots)
        return logs

    def _sample_host(self, prefix, length, context, variants, valid, args):
        '''the same chains on an engine without `sample_pick`: one `_predict_refs` per character and group, the picks of
        gensample.pick_host with the same uniform numbers; costs summed at the engine's own precision'''
        temperature, top_k, floor, seed = args
        i_c = self.mapping[1]
        state = None
        for char in prefix[:-1]:
            _, states = self._predict_refs([char], [state], context)
            state = states[0]
        logs = []
        for row0 in range(0, variants, gensample.MAX_ROWS):
            n = min(gensample.MAX_ROWS, variants - row0)
            chars, states = [prefix[-1]] * n, [state] * n
            idx_log = np.zeros((length, n), dtype=np.int32)
            cum_log = np.zeros((length, n), dtype=np.float64)
            u_log = np.zeros((length, n), dtype=np.float32)
            cum = np.zeros(n, dtype=np.float64)
            for s in range(length):
                probs, states = self._predict_refs(chars, states, context)
                u_log[s] = gensample.philox_uniform(seed, s, n, row0)
                idx_log[s] = gensample.pick_host(probs, u_log[s], valid, temperature, top_k, floor)
                with np.errstate(divide="ignore"):
                    cum = cum - np.log(np.asarray(probs)[np.arange(n), idx_log[s]].astype(np.float64))
                cum_log[s] = cum
                chars = [i_c[int(i)] for i in idx_log[s]]
            logs.append((idx_log, cum_log, u_log))
        return logs

    def rate_best(self, graph, start_node, end_node, start_traceback=None, context=None, lm_weight=0.5,
                  beam_width=10, beam_clustering_dist=0, edge_walk=None):
        '''Rate a lattice of string alternatives, decoding the best-scoring path
        incrementally (rating.py:712-859).  `graph` is a networkx.DiGraph whose edges
        carry `element` and `alternatives` (objects with `.Unicode`, `.conf`, `.index`).
        Returns (path [(element, alternative, score)], entropy, traceback).

        The beam bookkeeping lives in lattice_beam.py: one table of tracks per edge, list operations on track
        numbers and float keys, tree nodes only for the hypotheses that survive at an edge's destination.

        edge_walk (None: the attribute `self.edge_walk`): the characters an edge's hypotheses will feed are known in
        advance, so the model is asked ONCE per edge -- all hypotheses over all their characters in one engine call
        (HipLM.walk_host; an engine without it: chained steps) -- and the unchanged bookkeeping then reads the probabilities
        from that table (lattice_beam.walk_edge).  Same paths and costs; what it saves is the host round trip per character.'''
        if not context:
            context = self.underspecify_contexts()
        self._ensure_precision()
        if not start_traceback:
            root = Node(state=None, value='\n', cost=0.0)
            start_traceback = ([root], root)
        graph.nodes[start_node]['traceback'] = start_traceback[0]
        clustering = bool(beam_clustering_dist)

        def predict(chars, states, targets=None):
            return self._predict_refs(chars, states, context, heads=clustering, targets=targets)

        def close_states(a, b):
            return all(self._state_distance_below(a, b, k, beam_clustering_dist) for k in range(self.depth))

        if edge_walk is None:
            edge_walk = self.edge_walk
        walk = getattr(self.model, "walk_host", None) if edge_walk else None
        walk_ctx = np.asarray(windows.clamp_context(context), dtype=np.int32) if walk is not None else None
        reached = None
        for source, reached in lattice_beam.lattice_edges(graph, start_node):
            edge = graph.edges[source, reached]
            element, alternatives = edge['element'], edge['alternatives']
            self.logger.debug("rating %d alternatives from %d to %d", len(alternatives), source, reached)
            assert 'traceback' in graph.nodes[source], \
                "breadth-first search should have visited %d first in '%s'" % (source, element.id)
            target = graph.nodes[reached]
            tracks = lattice_beam.EdgeTracks(graph.nodes[source]['traceback'], alternatives, element, self.mapping[0],
                                             lm_weight, self.logger)
            finished = lattice_beam.FinishedBeam(target.get('traceback', []))
            table = None
            if edge_walk:
                table = lattice_beam.walk_edge(tracks, walk, pool=self._state_pool() if walk is not None else None, ctx=walk_ctx,
                                               head_k=self.depth if clustering else 0, slot_budget=self.edge_walk_slots,
                                               predict=predict)
            lattice_beam.decode_edge(tracks, finished, predict, self.batch_size,
                                     max(len(a.Unicode) for a in alternatives) * 3,
                                     close_states if clustering else None, table=table)
            target['traceback'] = [ref if kind == "node" else tracks.node(ref) for kind, ref in finished.items[:beam_width]]
        assert reached == end_node, \
            'breadth-first search failed to reach true end node (%s instead of %d)' % (reached, end_node)
        assert 'traceback' in graph.nodes[reached], \
            "breadth-first search failed to reach end node with any result"
        return self.next_path(graph.nodes[reached]['traceback'], start_traceback)

    def rate_best_batch(self, graphs, start_nodes, end_nodes, start_tracebacks=None, contexts=None, lm_weight=0.5,
                        beam_width=10, beam_clustering_dist=0, slot_budget_bytes=None):
        '''`rate_best(..., edge_walk=True)` for many independent lattices at once: returns [(path, entropy, traceback)] in
        input order, entry i what the single call returns for graphs[i] alone (the same `Node` trees: `next_path` and a
        carried traceback work unchanged; pass the returned tracebacks as `start_tracebacks` for every chain's next page).

        The lattices advance in lockstep (lattice_batch.py): round r takes the r-th edge of every lattice that still has
        one, all those edges' hypotheses are walked in ONE engine call and their beam bookkeeping runs in ONE more --
        on the device (HipLM.edge_round: kl_edge_costs + kl_edge_decode, one host wait per round), or, on an engine
        without it, as the plain function that defines the kernel (lattice_batch.edge_decode_host).
        contexts: None, one list for all lattices, or one list per lattice.  slot_budget_bytes: HBM one round's walk may
        take for the states between characters (None: lattice_batch.BATCH_SCRATCH_BYTES, 1 GiB -- 131072 states at
        depth 2, width 512); a round that needs more is walked in several calls.
        Unmapped characters are reported per edge in alternative order, the same set of messages as the single call.'''
        from . import lattice_batch
        return lattice_batch.decode_lattices(self, graphs, start_nodes, end_nodes, start_tracebacks, contexts, lm_weight,
                                             beam_width, beam_clustering_dist, slot_budget_bytes)

    def next_path(self, beam, traceback):
        '''Advance from `traceback` to `beam` (rating.py:862-885): lock into the best
        hypothesis' ancestor in the previous beam, emit its path, cut the others.'''
        return lattice_beam.advance_traceback(beam, traceback)

    def _state_distance_below(self, a, b, k, distance):
        if isinstance(a, StateRef) and isinstance(b, StateRef):
            if a.head is not None and b.head is not None:
                d = a.head[k] - b.head[k]
                return float(np.dot(d, d)) < distance * distance
            d2 = float(_np(self.model.state_dist2([a.slot], [b.slot], k))[0])
            return d2 < distance * distance
        return np.linalg.norm(np.asarray(a[k]) - np.asarray(b[k])) < distance

    # ------------------------------------------------------------------ model I/O
    def save(self, filename):
        '''Save weights and configuration (rating.py:918-945).'''
        assert self.status > 1
        config = {
            'history': json.dumps(self.history, cls=modelio.NumpyEncoder),
            'width': int(self.width), 'depth': int(self.depth), 'length': int(self.length),
            'stateful': bool(self.stateful), 'variable_length': bool(self.variable_length),
            'mapping': np.fromiter((ord(self.mapping[1][i]) if i in self.mapping[1] else 0
                                    for i in range(self.voc_size)), dtype='uint32'),
        }
        modelio.save_model(filename, self.model.get_weights(), config, self.depth, self.n_ctx)

    def load_config(self, filename):
        '''Load parameters to prepare configuration (rating.py:947-964).'''
        assert self.status == 0
        config = modelio.load_config(filename)
        history = config.get('history')
        self.history = json.loads(history) if history else {}
        self.width = int(config['width'])
        self.depth = int(config['depth'])
        self.length = int(config['length'])
        self.stateful = bool(config['stateful'])
        self.variable_length = bool(config['variable_length'])
        mapping = config['mapping']
        c_i = dict((chr(c), i) for i, c in enumerate(mapping) if c > 0)
        i_c = dict((i, chr(c)) for i, c in enumerate(mapping) if c > 0)
        self.mapping = (c_i, i_c)
        self.voc_size = len(c_i) + 1

    def load_weights(self, filename):
        '''Load weights into the configured model (rating.py:966-974).'''
        assert self.status > 0
        weights = modelio.load_weights(filename, self.depth, self.width, self.n_ctx)
        self.model.set_weights(weights, PREC_SPLIT)      # (rating needs the f32-accurate mode; train() re-prepares in bf16)
        self.status = 2

    # ---- offline views of the embeddings (rating.py:1169-1237; matplotlib / scikit-learn are imported on use)
    def _embedding(self, name):
        assert self.status == 2
        weights = self.model.get_weights()
        if name not in weights:
            raise KeyError("the model has no embedding '%s'" % name)
        return np.asarray(weights[name], dtype=np.float64)

    def plot_char_embeddings_similarity(self, filename):
        '''Paint a heat map of character embeddings: |E E^T| as a grayscale PNG (rating.py:1169-1187).'''
        import logging
        logging.getLogger('matplotlib').setLevel(logging.WARNING)
        from matplotlib import pyplot as plt
        from matplotlib import cm
        charwgt = self._embedding('E')
        plt.imsave(filename, np.abs(np.dot(charwgt, charwgt.T)), cmap=cm.gray)

    def plot_context_embeddings_similarity(self, filename, n=1):
        '''Paint a heat map of the n-th context variable's embeddings (rating.py:1189-1207).'''
        import logging
        logging.getLogger('matplotlib').setLevel(logging.WARNING)
        from matplotlib import pyplot as plt
        from matplotlib import cm
        ctxtwgt = self._embedding('Ctx%d' % (n - 1))
        plt.imsave(filename, np.abs(np.dot(ctxtwgt, ctxtwgt.T)), cmap=cm.gray)

    def plot_context_embeddings_projection(self, filename, n=1):
        '''Scatter plot of a 2-d PCA projection of the n-th context variable's embeddings, every point
        labelled with its decade (rating.py:1209-1237).  Labels are de-overlapped when adjustText is there.'''
        import logging
        logging.getLogger('matplotlib').setLevel(logging.WARNING)
        import matplotlib
        matplotlib.use('Agg')
        from matplotlib import pyplot as plt
        from sklearn.decomposition import PCA
        ctxtprj = PCA(n_components=2).fit_transform(self._embedding('Ctx%d' % (n - 1)))
        plt.figure(figsize=(11.7, 8.3))
        plt.plot(ctxtprj[:, 0], ctxtprj[:, 1], 'bo', markersize=2)
        texts = [plt.text(xy[0], xy[1], str(year) + 'x', c='b', size='xx-small') for year, xy in enumerate(ctxtprj)]
        try:
            from adjustText import adjust_text
            adjust_text(texts, time_lim=20, iter_lim=20, expand_axes=True, arrowprops=dict(arrowstyle="-", color='b', lw=0.5))
        except ImportError:
            pass
        plt.tick_params(left=False, right=False, bottom=False, labelleft=False, labelbottom=False)
        plt.savefig(filename)
        plt.close()

    def print_charset(self):
        '''Print the mapped characters (rating.py:1160-1167).'''
        import unicodedata
        for i, c in self.mapping[1].items():
            print('%d: "%s"' % (i, c))
            char = unicodedata.normalize('NFC', c)
            if c != char:
                self.logger.warning('mapped character "%s" (%d) should have been normalized to "%s", which is %s mapped',
                                    c, i, char, 'also' if char in self.mapping[0] else 'not')
