# -*- coding: utf-8 -*-
"""`keraslm-rate` command line (drop-in for ocrd_keraslm/scripts/run.py:31-221).

Same commands, options, defaults and outputs as the reference CLI: train, test,
apply, generate, print-history, print-charset, prune-charset and the three plot-* views of the
embeddings (matplotlib / scikit-learn imported on use).
Additional command `score`: bits per character and perplexity of every DATA file, all files rated at once
(Rater.rate_batch; --precision bf16 takes the bulk path on the training forward).
Additional command `suspects`: per DATA file the characters the model does not believe, with what it expected instead
(Rater.suspects: rated in bulk, picked out on the device).
Additional command `correct`: the suspects of every DATA file with their alternatives rescored against the text that follows,
and what that proposes to write instead (Rater.corrections); --deletions also tries dropping the character, --insertions a
lost character in front of it, --share-left reads a suspect's left context once for all of these; --apply also gives the
corrected text.
Additional command `rescore`: replacements that come from outside the model -- per-file candidate lists (--candidates) or a
table of known confusions (--confusions, gated by a `suspects` pass) -- rated against the text around their spans
(Rater.rescore); --apply also gives the corrected text.
Additional command `contexts`: per DATA file the context it reads like among the candidates given (--years or --candidates),
the posterior over them, and its bits under the best one, under their sequential mixture and under context 0
(Rater.rate_contexts: every file under every candidate in one bulk plan).
Additional command `words`: per DATA file the words the model does not believe -- at least --min-suspects suspect characters,
--min-bits-per-char bits per predicted character and --min-chars predicted characters -- with their bits, mean and least
probability (Rater.suspect_words: rated in bulk, the words found, rated and picked out on the device).
Additional command `lexicon`: the suspect words of every DATA file looked up in a word list (--lexicon, the most frequent entry
first) on the device, and their nearest entries rated against the text around them (Rater.correct_words: suspect_words ->
lexicon_neighbours -> rescore); output as `rescore`'s, --apply also gives the corrected text.  With --channel FILE (the JSON
lines of `confusions --counts`) the look-up weighs the learned confusions and their bits enter the choice (Rater.channel).
With --boundaries lost and spurious spaces are hypotheses too: a word as two entries (Rater.lexicon_splits), two words as one;
with --max-parts N a word as up to N entries, and with --compounds N a chain of 2 .. N entries is left alone (Rater.lexicon_chains).
Additional command `witnesses`: every DATA file aligned with other readings of it (--witness DIR: the file of the same base
name) on the device, and the readings of the spans where they differ rated against the text around them
(Rater.merge_witnesses: align -> witness_edits -> rescore); --apply also gives the corrected text.
Additional command `confusions`: every DATA file (OCR output) aligned with its ground truth (--truth DIR: the file of the same
base name) on the device, and the differences counted there into a table of confusions -- which strings were read as which, how
often, and how often the source stands in the OCR at all (Rater.confusions: align_pairs -> confusion_counts); the table goes to
stdout as the TSV that `rescore --confusions` reads, or with --counts as one JSON line per record; pairs, skipped spans and the
character error rate go to stderr.
Additional command `consensus`: `witnesses` for files with several witnesses -- the witnesses' differences clustered across
witnesses on the device, so that overlapping differences are one hypothesis, every witness read over a whole cluster, equal
readings counted (Rater.consensus: align_pairs -> witness_clusters -> the rating of `rescore`); --vote-bits weighs a witness'
vote against the model's bits; the votes stand beside every rescored span, --apply also gives the corrected text.
Additional options on `train`: --streams (stateful streams per GPU, default 1 = the
reference's batching) and --segment-streams (with fewer files than streams, cut the files
into contiguous segments on window boundaries, one list of segments per stream).  Under `python -m torch.distributed.run` training is
data-parallel over the launched ranks (lib/distributed.py).
"""
from __future__ import absolute_import

import json
import os
import sys
from math import ceil

import click

from .. import lib

COMMAND_ORDER = ['train', 'test', 'score', 'suspects', 'correct', 'rescore', 'contexts', 'words', 'lexicon', 'witnesses', 'confusions', 'consensus', 'apply', 'generate', 'print-history', 'print-charset', 'prune-charset',
                 'plot-char-embeddings-similarity', 'plot-context-embeddings-similarity', 'plot-context-embeddings-projection']


class OrderedGroup(click.Group):
    def list_commands(self, ctx):
        names = list(super(OrderedGroup, self).list_commands(ctx))
        return [n for n in COMMAND_ORDER if n in names] + sorted(n for n in names if n not in COMMAND_ORDER)


@click.group(cls=OrderedGroup)
def cli():
    pass


def _open_all(items):
    """files, or every regular file of a directory (run.py:70-80, 124-131)"""
    handles = []
    for item in items:
        if os.path.isdir(item):
            paths = [os.path.join(item, name) for name in os.listdir(item)]
            handles.extend(open(p, mode='r') for p in paths if os.path.isfile(p))
        else:
            handles.append(open(item, mode='r'))
    return handles


def _contexts(text):
    """'1784' -> [179]: one context id = ceil(year/10) per blank-separated number (run.py:105-106)"""
    return [ceil(int(x) / 10) for x in text.split(' ')]


def _load(model, incremental=False):
    rater = lib.Rater()
    rater.load_config(model)
    if incremental:
        rater.stateful = False
        rater.incremental = True
    rater.configure()
    rater.load_weights(model)
    return rater


@cli.command(short_help='train a language model')
@click.option('-m', '--model', default="model.h5", show_default=True, help='model file',
              type=click.Path(dir_okay=False, writable=True))
@click.option('-C', '--ckpt', default="ckpt.h5", show_default=True, help='checkpoint file', type=click.Path(dir_okay=False))
@click.option('-w', '--width', default=128, show_default=True, help='number of nodes per hidden layer',
              type=click.IntRange(min=1, max=9128))
@click.option('-d', '--depth', default=2, show_default=True, help='number of hidden layers', type=click.IntRange(min=1, max=10))
@click.option('-l', '--length', default=256, show_default=True, help='number of previous characters seen (window size)',
              type=click.IntRange(min=1, max=1024))
@click.option('-v', '--val-data', default=None, show_default=True,
              help='validation data file or directory (instead of automatic split)',
              type=click.Path(exists=True, dir_okay=True, file_okay=True))
@click.option('-s', '--streams', default=1, show_default=True, help='stateful streams trained in lockstep per GPU',
              type=click.IntRange(min=1, max=4096))
@click.option('--segment-streams', is_flag=True, default=False,
              help='with fewer files than streams, cut the files into segments (on window boundaries) and deal those')
@click.argument('data', nargs=-1, type=click.Path(exists=True, dir_okay=True, file_okay=True))
def train(model, ckpt, width, depth, length, val_data, streams, segment_streams, data):
    """Train a language model from DATA files,
       with parameters WIDTH, DEPTH, and LENGTH.

       The files will be randomly split into training and validation data,
       except if VAL_DATA is given.
    """
    from ..lib.distributed import init_from_env
    rank, _world, _local = init_from_env()
    rater = lib.Rater()
    resume = None
    if os.path.isfile(model):
        rater.load_config(model)
        if rater.width == width and rater.depth == depth:
            resume = model
            print('loading weights from existing model for continued training')
        else:
            print('warning: ignoring existing model due to different topology (width=%d, depth=%d)'
                  % (rater.width, rater.depth), file=sys.stderr)
    elif os.path.isfile(ckpt):
        resume = ckpt
        print('loading weights from checkpoint for continued training')
    rater.width, rater.depth, rater.length = width, depth, length
    rater.streams = streams
    rater.segment_streams = segment_streams
    rater.configure()
    if resume:
        if rater.model is None:
            # a bare checkpoint carries no mapping (latent bugs): nothing to resume into
            print('warning: cannot resume from %s without a character mapping' % resume, file=sys.stderr)
        else:
            rater.load_weights(resume)
    training = _open_all(data)
    validation = _open_all([val_data]) if val_data else None
    rater.train(training, val_data=validation)
    assert rater.status == 2
    if rank == 0:
        rater.save(model)


@cli.command(short_help='get individual probabilities from language model')
@click.option('-m', '--model', required=True, help='model file', type=click.Path(dir_okay=False, exists=True))
@click.option('-c', '--context', default=None, help='constant meta-data input')
@click.option('--alternatives', default=None, type=click.IntRange(min=1, max=8),
              help='also list the K characters the model expected most at every position, and the rank of the one written')
@click.argument('text', type=click.STRING)
def apply(model, text, context, alternatives):
    """Apply a language model to TEXT string and compute its individual probabilities.

       If TEXT is the symbol '-', the string will be read from standard input.

       With --alternatives K the list holds [char, prob, rank, [[alt_char, alt_prob], ...]]
       per character (rank 0: the model's first choice; the first character has no prediction).
    """
    rater = _load(model)
    if text and text[0] == u"-":
        text = sys.stdin.read()
    if alternatives:
        from ..lib import windows
        rated, bits = rater.rate_alternatives([text], [_contexts(context)] if context else None, k=alternatives)
        text = windows.normalize(text)
        one = rated[0]
        click.echo(pow(2.0, float(bits[0]) / max(len(text), 1)))
        click.echo(json.dumps([[char, float(one.probs[i]), int(one.rank[i]),
                                [[c, float(p)] for c, p in zip(chars, one.alt_probs[i])]]
                               for i, (char, chars) in enumerate(zip(text, one.chars(rater.mapping)))], ensure_ascii=False))
        return
    ratings, perplexity = rater.rate2(text, _contexts(context) if context else None)
    click.echo(perplexity)
    click.echo(json.dumps(ratings, ensure_ascii=False))


@cli.command(short_help='get overall perplexity from language model')
@click.option('-m', '--model', required=True, help='model file', type=click.Path(dir_okay=False, exists=True))
@click.argument('data', nargs=-1, type=click.Path(exists=True, dir_okay=True, file_okay=True))
def test(model, data):
    """Apply a language model to DATA files and compute its overall perplexity."""
    rater = _load(model)
    click.echo(rater.test(_open_all(data)))


@cli.command(short_help='get bits per character and perplexity of every file')
@click.option('-m', '--model', default="model.h5", show_default=True, help='model file', type=click.Path(dir_okay=False, exists=True))
@click.option('-s', '--streams', default=64, show_default=True, help='files rated in lockstep, one per row of a window call',
              type=click.IntRange(min=1, max=4096))
@click.option('--precision', default='split', show_default=True, type=click.Choice(['split', 'bf16']),
              help='split: the inference kernels, ~f32 accuracy; bf16: bulk rating on the training forward '
                   '(probabilities within 1e-2, several times the throughput on many files)')
@click.argument('data', nargs=-1, type=click.Path(exists=True, dir_okay=True, file_okay=True))
def score(model, streams, precision, data):
    """Apply a language model to DATA files and print one JSON line per file:
       characters, bits per character and perplexity.

       Every file is rated on its own, from a zero state (unlike `test`, which carries the
       state from file to file); its context comes from its name, as in `test` and `train`.
    """
    from ..lib import windows
    rater = _load(model)
    names, texts, contexts = [], [], []
    for file in _open_all(data):
        with file:
            texts.append(windows.normalize(file.read()))
        names.append(file.name)
        contexts.append(windows.context_from_filename(file.name))
    if not texts:
        return
    _, bits = rater.rate_batch(texts, contexts, streams=streams, want_probs=False, precision=precision)
    for name, text, total in zip(names, texts, bits):
        per_char = float(total) / max(len(text) - 1, 1)
        click.echo(json.dumps({"file": name, "chars": len(text), "bits_per_char": per_char, "perplexity": 2.0 ** per_char},
                              ensure_ascii=False))


@cli.command(short_help='list the characters of every file that the model does not believe')
@click.option('-m', '--model', default="model.h5", show_default=True, help='model file', type=click.Path(dir_okay=False, exists=True))
@click.option('-s', '--streams', default=1024, show_default=True, help='files rated in lockstep, one per row of a window call',
              type=click.IntRange(min=1, max=4096))
@click.option('--precision', default='bf16', show_default=True, type=click.Choice(['bf16', 'split']),
              help='bf16: bulk rating on the training forward; split: the inference kernels, ~f32 accuracy')
@click.option('-k', 'k', default=3, show_default=True, type=click.IntRange(min=1, max=8),
              help='characters the model expected most, listed per suspect')
@click.option('--max-prob', default=0.01, show_default=True, type=click.FLOAT,
              help='a suspect has at most this probability')
@click.option('--min-rank', default=1, show_default=True, type=click.IntRange(min=0),
              help='... and at least this rank among the characters the model could have written (0: its first choice)')
@click.argument('data', nargs=-1, type=click.Path(exists=True, dir_okay=True, file_okay=True))
def suspects(model, streams, precision, k, max_prob, min_rank, data):
    """Apply a language model to DATA files and print one JSON line per file: characters, bits per
       character and the suspect characters as [position, char, prob, rank, [[alt_char, alt_prob], ...]].

       Files are read, and given their contexts, as `score` does.  Only the suspects leave the device.
    """
    from ..lib import windows
    rater = _load(model)
    names, texts, contexts = [], [], []
    for file in _open_all(data):
        with file:
            texts.append(windows.normalize(file.read()))
        names.append(file.name)
        contexts.append(windows.context_from_filename(file.name))
    if not texts:
        return
    found, bits = rater.suspects(texts, contexts, k=k, streams=streams, max_prob=max_prob, min_rank=min_rank,
                                 precision=precision)
    for name, text, one, total in zip(names, texts, found, bits):
        rows = [[int(j), text[int(j)], float(p), int(r), [[c, float(q)] for c, q in zip(chars, probs)]]
                for j, p, r, chars, probs in zip(one.positions, one.probs, one.rank, one.chars(rater.mapping), one.alt_probs)]
        click.echo(json.dumps({"file": name, "chars": len(text), "bits_per_char": float(total) / max(len(text) - 1, 1),
                               "suspects": rows}, ensure_ascii=False))


@cli.command(short_help='propose corrections for the characters of every file that the model does not believe')
@click.option('-m', '--model', default="model.h5", show_default=True, help='model file', type=click.Path(dir_okay=False, exists=True))
@click.option('-s', '--streams', default=1024, show_default=True, help='rows of a window call: files in the first pass, hypotheses in the second',
              type=click.IntRange(min=1, max=4096))
@click.option('--precision', default='bf16', show_default=True, type=click.Choice(['bf16', 'split']),
              help='bf16: bulk rating on the training forward; split: the inference kernels, ~f32 accuracy')
@click.option('-k', 'k', default=3, show_default=True, type=click.IntRange(min=1, max=8),
              help='characters the model expected most, tried per suspect')
@click.option('--max-prob', default=0.01, show_default=True, type=click.FLOAT,
              help='a suspect has at most this probability')
@click.option('--min-rank', default=1, show_default=True, type=click.IntRange(min=0),
              help='... and at least this rank among the characters the model could have written (0: its first choice)')
@click.option('--left', default=64, show_default=True, type=click.IntRange(min=1, max=1024),
              help='characters in front of a suspect that a hypothesis is read from (from a zero state)')
@click.option('--ahead', default=8, show_default=True, type=click.IntRange(min=0, max=1023),
              help='characters after a suspect that a hypothesis is held against')
@click.option('--deletions', is_flag=True, default=False, help='also try dropping the suspect character')
@click.option('--insertions', is_flag=True, default=False,
              help='also try each expected character in front of the suspect: a character the text has lost')
@click.option('--min-gain', default=1.0, show_default=True, type=click.FLOAT,
              help='a proposal must save at least this many bits against the text as written')
@click.option('--share-left', is_flag=True, default=False,
              help='read the LEFT characters once per suspect instead of once per hypothesis (suspects with fewer than LEFT '
                   'characters in front of them are not shared: on short lines choose a smaller --left)')
@click.option('--apply', 'apply_', is_flag=True, default=False, help='also give the text with the proposals applied ("corrected")')
@click.argument('data', nargs=-1, type=click.Path(exists=True, dir_okay=True, file_okay=True))
def correct(model, streams, precision, k, max_prob, min_rank, left, ahead, deletions, insertions, min_gain, share_left, apply_,
            data):
    """Apply a language model to DATA files and print one JSON line per file, as `suspects` does, with
       "corrections": one [position, written, proposed, gain] per suspect -- proposed is what replaces the
       written character: null for no proposal, "" for dropping it, one character for another in its place
       and (--insertions) two for a lost character in front of it; gain the bits the proposal saves over the
       LEFT characters in front of the suspect and the AHEAD characters after it.  With --apply the line also
       holds the corrected text.
    """
    from ..lib import windows
    if left + ahead + int(insertions) > 1024:
        raise click.UsageError("--left + --ahead%s must not exceed 1024" % (" + 1 (--insertions)" if insertions else ""))
    rater = _load(model)
    names, texts, contexts = [], [], []
    for file in _open_all(data):
        with file:
            texts.append(windows.normalize(file.read()))
        names.append(file.name)
        contexts.append(windows.context_from_filename(file.name))
    if not texts:
        return
    found, bits = rater.corrections(texts, contexts, k=k, streams=streams, max_prob=max_prob, min_rank=min_rank, left=left,
                                    ahead=ahead, deletions=deletions, min_gain=min_gain, precision=precision,
                                    insertions=insertions, share_left=share_left)
    for name, text, one, total in zip(names, texts, found, bits):
        rows = [[int(j), text[int(j)], float(p), int(r), [[c, float(q)] for c, q in zip(chars, probs)]]
                for j, p, r, chars, probs in zip(one.positions, one.probs, one.rank, one.chars(rater.mapping), one.alt_probs)]
        proposals = [[int(j), text[int(j)], new, float(g)]
                     for j, new, g in zip(one.positions, one.edits(text, rater.mapping), one.gain)]
        line = {"file": name, "chars": len(text), "bits_per_char": float(total) / max(len(text) - 1, 1), "suspects": rows,
                "corrections": proposals}
        if apply_:
            line["corrected"] = one.apply(text, rater.mapping)
        click.echo(json.dumps(line, ensure_ascii=False))


def _read_confusions(path):
    """TSV lines `source<TAB>replacement[<TAB>replacement ...]` -> [(source, [replacements])]; an empty field drops the source"""
    rules = []
    with open(path, mode='r') as file:
        for number, line in enumerate(file, 1):
            line = line.rstrip('\n').rstrip('\r')
            if not line:
                continue
            fields = line.split('\t')
            if not fields[0] or len(fields) < 2:
                raise click.UsageError("%s:%d: a source and at least one replacement, separated by tabs" % (path, number))
            rules.append((fields[0], fields[1:]))
    return rules


def _read_candidates(path, names):
    """JSON lines {"file", "start", "end", "candidates"} -> edits for Rater.rescore over the files `names`"""
    index = dict((name, i) for i, name in enumerate(names))
    edits = []
    with open(path, mode='r') as file:
        for number, line in enumerate(file, 1):
            if not line.strip():
                continue
            try:
                one = json.loads(line)
                edits.append((index[one["file"]], int(one["start"]), int(one["end"]), [str(c) for c in one["candidates"]]))
            except (ValueError, KeyError, TypeError) as err:
                raise click.UsageError("%s:%d: %r (a JSON object with \"file\" -- one of DATA --, \"start\", \"end\", "
                                       "\"candidates\")" % (path, number, err))
    return edits


@cli.command(short_help='rate replacements from outside the model for spans of every file')
@click.option('-m', '--model', default="model.h5", show_default=True, help='model file', type=click.Path(dir_okay=False, exists=True))
@click.option('-s', '--streams', default=1024, show_default=True, help='rows of a window call: hypotheses (files in the pass of --confusions)',
              type=click.IntRange(min=1, max=4096))
@click.option('--precision', default='bf16', show_default=True, type=click.Choice(['bf16', 'split']),
              help='bf16: bulk rating on the training forward; split: the inference kernels, ~f32 accuracy')
@click.option('--left', default=64, show_default=True, type=click.IntRange(min=1, max=1024),
              help='characters in front of a span that a hypothesis is read from (from a zero state)')
@click.option('--ahead', default=8, show_default=True, type=click.IntRange(min=0, max=1023),
              help='characters after a span that a hypothesis is held against')
@click.option('--min-gain', default=1.0, show_default=True, type=click.FLOAT,
              help='a proposal must save at least this many bits against the text as written')
@click.option('--apply', 'apply_', is_flag=True, default=False, help='also give the text with the proposals applied ("corrected")')
@click.option('--candidates', default=None, type=click.Path(dir_okay=False, exists=True),
              help='JSON lines {"file", "start", "end", "candidates"}: replacement strings for the span [start, end) of a DATA file')
@click.option('--confusions', default=None, type=click.Path(dir_okay=False, exists=True),
              help='TSV lines: a source string, then its replacements (an empty field drops the source); tried at the '
                   'occurrences that hold a suspect character')
@click.option('-k', 'k', default=3, show_default=True, type=click.IntRange(min=1, max=8),
              help='(--confusions) alternatives of the suspects pass')
@click.option('--max-prob', default=0.01, show_default=True, type=click.FLOAT,
              help='(--confusions) a suspect has at most this probability')
@click.option('--min-rank', default=1, show_default=True, type=click.IntRange(min=0),
              help='(--confusions) ... and at least this rank; --max-prob 1 --min-rank 0 keeps every occurrence')
@click.argument('data', nargs=-1, type=click.Path(exists=True, dir_okay=True, file_okay=True))
def rescore(model, streams, precision, left, ahead, min_gain, apply_, candidates, confusions, k, max_prob, min_rank, data):
    """Apply a language model to DATA files and print one JSON line per file: characters and
       "rescored": one [start, end, written, proposed, gain] per span -- proposed is what replaces
       text[start:end]: null for no proposal, "" for dropping it; gain the bits the proposal saves over the
       span and the AHEAD characters after it, read after the LEFT characters in front.  The replacements
       come from --candidates or from --confusions (exactly one of them).  With --apply the line also
       holds the corrected text.
    """
    from ..lib import ratebatch, windows
    if (candidates is None) == (confusions is None):
        raise click.UsageError("exactly one of --candidates and --confusions")
    rules = _read_confusions(confusions) if confusions is not None else None
    rater = _load(model)
    names, texts, contexts = [], [], []
    for file in _open_all(data):
        with file:
            texts.append(windows.normalize(file.read()))
        names.append(file.name)
        contexts.append(windows.context_from_filename(file.name))
    if not texts:
        return
    if rules is not None:
        found, _ = rater.suspects(texts, contexts, k=k, streams=streams, max_prob=max_prob, min_rank=min_rank, precision=precision)
        edits = ratebatch.confusion_edits(texts, rules, at=[one.positions for one in found])
    else:
        edits = _read_candidates(candidates, names)
    try:
        found = rater.rescore(texts, edits, contexts, streams=streams, left=left, ahead=ahead, min_gain=min_gain,
                              precision=precision, want_costs=False)
    except ValueError as err:
        raise click.UsageError(str(err))
    for name, text, one in zip(names, texts, found):
        rows = [[int(a), int(b), text[int(a):int(b)], new, float(g)]
                for a, b, new, g in zip(one.starts, one.ends, one.proposals(), one.gain)]
        line = {"file": name, "chars": len(text), "rescored": rows}
        if apply_:
            line["corrected"] = one.apply(text)
        click.echo(json.dumps(line, ensure_ascii=False))


def _year_candidates(spec):
    """'1700:1900:10' -> the distinct context ids of the years FROM, FROM + STEP, .. up to TO (STEP 10 if left out), as
    `_contexts` maps them, in ascending order of the years"""
    parts = spec.split(':')
    if len(parts) not in (2, 3):
        raise click.BadParameter('FROM:TO[:STEP]', param_hint='--years')
    try:
        first, last = int(parts[0]), int(parts[1])
        step = int(parts[2]) if len(parts) == 3 else 10
    except ValueError:
        raise click.BadParameter('FROM:TO[:STEP] in whole years', param_hint='--years')
    if step < 1 or last < first:
        raise click.BadParameter('FROM <= TO and STEP >= 1', param_hint='--years')
    out = []
    for year in range(first, last + 1, step):
        c = _contexts(str(year))
        if c not in out:
            out.append(c)
    return out


def _read_context_candidates(path):
    """one blank-separated context tuple per line, in the notation `apply -c` takes (years); empty lines are skipped"""
    with open(path, mode='r') as file:
        return [_contexts(' '.join(line.split())) for line in file if line.strip()]


@cli.command(short_help='find the context every file reads like, and rate it under the mixture of the candidates')
@click.option('-m', '--model', default="model.h5", show_default=True, help='model file', type=click.Path(dir_okay=False, exists=True))
@click.option('-s', '--streams', default=1024, show_default=True, help='rows of a window call: pairs of a file and a candidate',
              type=click.IntRange(min=1, max=4096))
@click.option('--precision', default='bf16', show_default=True, type=click.Choice(['bf16', 'split']),
              help='bf16: bulk rating on the training forward; split: the inference kernels, ~f32 accuracy')
@click.option('--years', default=None, help='FROM:TO[:STEP]: one candidate per decade of these years (models of one context variable)')
@click.option('--candidates', default=None, type=click.Path(dir_okay=False, exists=True),
              help='file with one candidate per line: blank-separated meta-data as `apply -c` takes it')
@click.option('--top', default=3, show_default=True, type=click.IntRange(min=1, max=256), help='posteriors listed per file')
@click.argument('data', nargs=-1, type=click.Path(exists=True, dir_okay=True, file_okay=True))
def contexts(model, streams, precision, years, candidates, top, data):
    """Apply a language model to DATA files under every candidate context and print one JSON line per file:
       characters, the most probable candidate and its margin in bits, the --top candidates with their
       posteriors (uniform prior), and bits per character under the best candidate, under the sequential
       mixture of all of them and -- if it is not a candidate itself -- under context 0, the rating a
       caller gets today who does not know the context.

       Files are read as `score` reads them; their names are not asked for a context.
    """
    from ..lib import windows
    if (years is None) == (candidates is None):
        raise click.UsageError('give either --years or --candidates')
    rater = _load(model)
    if years is not None:
        if rater.n_ctx != 1:
            raise click.UsageError('--years is for models of one context variable (this one has %d)' % rater.n_ctx)
        cands = _year_candidates(years)
    else:
        cands = _read_context_candidates(candidates)
    cands = [windows.clamp_context(c) for c in cands]
    names, texts = [], []
    for file in _open_all(data):
        with file:
            texts.append(windows.normalize(file.read()))
        names.append(file.name)
    if not texts:
        return
    # context 0 is one more candidate of the same call, kept out of the posterior and the mixture by a zero prior
    zero = [0] * rater.n_ctx
    prior = None
    if zero not in cands:
        prior = [1.0] * len(cands) + [0.0]
    found = rater.rate_contexts(texts, cands + ([zero] if prior else []), prior=prior, streams=streams, precision=precision,
                                want_probs=False)
    for name, text, one in zip(names, texts, found):
        preds = max(len(text) - 1, 1)
        order = sorted(range(len(cands)), key=lambda c: (-one.posterior[c], c))[:top]
        line = {"file": name, "chars": len(text), "best": cands[one.best], "margin_bits": None if one.margin == float("inf") else one.margin,      # (None: no other candidate)
                "top": [[cands[c], float(one.posterior[c])] for c in order],
                "bits_per_char": float(one.bits[one.best]) / preds, "bits_per_char_mixture": one.mix_bits / preds}
        if prior:
            line["bits_per_char_context0"] = float(one.bits[-1]) / preds
        click.echo(json.dumps(line, ensure_ascii=False))


@cli.command(short_help='list the words of every file that the model does not believe')
@click.option('-m', '--model', default="model.h5", show_default=True, help='model file', type=click.Path(dir_okay=False, exists=True))
@click.option('-s', '--streams', default=1024, show_default=True, help='files rated in lockstep, one per row of a window call',
              type=click.IntRange(min=1, max=4096))
@click.option('--precision', default='bf16', show_default=True, type=click.Choice(['bf16', 'split']),
              help='bf16: bulk rating on the training forward; split: the inference kernels, ~f32 accuracy')
@click.option('-k', 'k', default=3, show_default=True, type=click.IntRange(min=1, max=8),
              help='alternatives ranked per character in the rating pass')
@click.option('--max-prob', default=0.01, show_default=True, type=click.FLOAT,
              help='a suspect character has at most this probability')
@click.option('--min-rank', default=1, show_default=True, type=click.IntRange(min=0),
              help='... and at least this rank among the characters the model could have written (0: its first choice)')
@click.option('--min-suspects', default=1, show_default=True, type=click.IntRange(min=0),
              help='a listed word has at least this many suspect characters')
@click.option('--min-bits-per-char', default=0.0, show_default=True, type=click.FloatRange(min=0.0),
              help='... at least this many bits per predicted character')
@click.option('--min-chars', default=1, show_default=True, type=click.IntRange(min=1),
              help='... and at least this many predicted characters')
@click.option('--delimiters', default=None, help='the characters that separate words [default: the mapped whitespace characters]')
@click.argument('data', nargs=-1, type=click.Path(exists=True, dir_okay=True, file_okay=True))
def words(model, streams, precision, k, max_prob, min_rank, min_suspects, min_bits_per_char, min_chars, delimiters, data):
    """Apply a language model to DATA files and print one JSON line per file: characters, bits per
       character and the suspect words as [start, word, n, bits, mean_prob, min_prob, worst, suspects].

       Files are read, and given their contexts, as `score` does.  Only the listed words leave the device.
    """
    from ..lib import windows
    rater = _load(model)
    names, texts, contexts = [], [], []
    for file in _open_all(data):
        with file:
            texts.append(windows.normalize(file.read()))
        names.append(file.name)
        contexts.append(windows.context_from_filename(file.name))
    if not texts:
        return
    found, bits = rater.suspect_words(texts, contexts, delimiters=delimiters, k=k, streams=streams, max_prob=max_prob,
                                      min_rank=min_rank, min_suspects=min_suspects, min_bits_per_char=min_bits_per_char,
                                      min_chars=min_chars, precision=precision)
    for name, text, one, total in zip(names, texts, found, bits):
        rows = [[int(a), word, int(n), float(b), float(mean), float(least), int(worst), int(bad)]
                for a, word, n, b, mean, least, worst, bad in zip(one.start, one.strings(text), one.n, one.bits, one.mean_prob,
                                                                  one.min_prob, one.worst, one.suspects)]
        click.echo(json.dumps({"file": name, "chars": len(text), "bits_per_char": float(total) / max(len(text) - 1, 1),
                               "words": rows}, ensure_ascii=False))


def _read_lexicon(path):
    """one entry per line, the most frequent first; anything after a tab (a count, say) is ignored"""
    with open(path, mode='r') as file:
        return [line.rstrip('\r\n').split('\t')[0] for line in file]


def _read_channel(path):
    """the JSON lines of `confusions --counts` as (source, target, count, occ); empty lines are skipped"""
    with open(path, mode='r') as file:
        records = [json.loads(line) for line in file if line.strip()]
    return [(r["source"], r["target"], r["count"], r["occ"]) for r in records]


@cli.command('lexicon', short_help='correct the words the model does not believe from a word list')
@click.option('-m', '--model', default="model.h5", show_default=True, help='model file', type=click.Path(dir_okay=False, exists=True))
@click.option('--lexicon', 'lexicon_file', required=True, type=click.Path(dir_okay=False, exists=True),
              help='word list: one entry per line, the most frequent first; anything after a tab is ignored')
@click.option('--max-dist', default=2, show_default=True, type=click.IntRange(min=0, max=8),
              help='an entry is a candidate for a word within this many edits (insertions, deletions, substitutions)')
@click.option('--per-word', default=8, show_default=True, type=click.IntRange(min=1, max=16),
              help='candidates per word at most: the nearest, the more frequent among equally near ones')
@click.option('--known', is_flag=True, default=False, help='also look up the words that are entries themselves')
@click.option('-s', '--streams', default=1024, show_default=True, help='rows of a window call: files, then hypotheses',
              type=click.IntRange(min=1, max=4096))
@click.option('--precision', default='bf16', show_default=True, type=click.Choice(['bf16', 'split']),
              help='bf16: bulk rating on the training forward; split: the inference kernels, ~f32 accuracy')
@click.option('-k', 'k', default=3, show_default=True, type=click.IntRange(min=1, max=8),
              help='alternatives ranked per character in the rating pass')
@click.option('--max-prob', default=0.01, show_default=True, type=click.FLOAT,
              help='a suspect character has at most this probability')
@click.option('--min-rank', default=1, show_default=True, type=click.IntRange(min=0),
              help='... and at least this rank among the characters the model could have written (0: its first choice)')
@click.option('--min-suspects', default=1, show_default=True, type=click.IntRange(min=0),
              help='a word is looked up with at least this many suspect characters')
@click.option('--min-bits-per-char', default=0.0, show_default=True, type=click.FloatRange(min=0.0),
              help='... at least this many bits per predicted character')
@click.option('--min-chars', default=1, show_default=True, type=click.IntRange(min=1),
              help='... and at least this many predicted characters')
@click.option('--delimiters', default=None, help='the characters that separate words [default: the mapped whitespace characters]')
@click.option('--left', default=64, show_default=True, type=click.IntRange(min=1, max=1024),
              help='characters in front of a word that a hypothesis is read from (from a zero state)')
@click.option('--ahead', default=8, show_default=True, type=click.IntRange(min=0, max=1023),
              help='characters after a word that a hypothesis is held against')
@click.option('--min-gain', default=1.0, show_default=True, type=click.FLOAT,
              help='a proposal must save at least this many bits against the text as written')
@click.option('--apply', 'apply_', is_flag=True, default=False, help='also give the text with the proposals applied ("corrected")')
@click.option('--channel', 'channel_file', default=None, type=click.Path(dir_okay=False, exists=True),
              help='table of confusions, the JSON lines of `confusions --counts`: the candidates of a word are the entries that are '
                   'cheap under these confusions (--max-dist is not used), and what they cost enters the choice')
@click.option('--unit-bits', default=8.0, show_default=True, type=click.FloatRange(min=0.0625, max=255.9),
              help='with --channel: bits of an insertion, deletion or substitution that no confusion explains')
@click.option('--max-bits', default=12.0, show_default=True, type=click.FloatRange(min=0.0, max=255.9),
              help='with --channel: an entry is a candidate for a word within this many bits')
@click.option('--channel-weight', default=1.0, show_default=True, type=click.FloatRange(min=0.0),
              help="with --channel: a candidate's bits under the channel count this much beside the model's (0: the model alone chooses)")
@click.option('--min-count', default=2, show_default=True, type=click.IntRange(min=0),
              help='with --channel: a confusion was seen at least this often')
@click.option('--min-rate', default=0.0, show_default=True, type=click.FLOAT,
              help='with --channel: ... and at no less than this share of the occurrences of its source')
@click.option('--boundaries', is_flag=True, default=False,
              help='also try word boundaries: a looked-up word as two entries with a space between them ("split"), and a '
                   'looked-up word run together with the word before or after it ("merge"); every record then ends with its kind')
@click.option('--min-part', default=2, show_default=True, type=click.IntRange(min=1, max=32),
              help='with --boundaries or --compounds: each part of a word has at least this many characters')
@click.option('--compounds', default=0, show_default=True, type=click.IntRange(min=0, max=8),
              help='a word that is a chain of 2 .. N entries (a compound) counts as an entry and is left alone [0: off]')
@click.option('--links', default=None,
              help='with --compounds: linking elements that may stand between two parts, separated by commas (s,es,n); '
                   'at most 8, of 1 .. 3 characters')
@click.option('--max-parts', default=2, show_default=True, type=click.IntRange(min=2, max=8),
              help='with --boundaries: also try a looked-up word as 3 .. N entries with spaces between them ("split")')
@click.argument('data', nargs=-1, type=click.Path(exists=True, dir_okay=True, file_okay=True))
def lexicon_(model, lexicon_file, max_dist, per_word, known, streams, precision, k, max_prob, min_rank, min_suspects,
             min_bits_per_char, min_chars, delimiters, left, ahead, min_gain, apply_, channel_file, unit_bits, max_bits,
             channel_weight, min_count, min_rate, boundaries, min_part, compounds, links, max_parts, data):
    """Apply a language model to DATA files, look the words it does not believe up in the word list and
       print one JSON line per file, as `rescore` does: characters and "rescored": one [start, end, written,
       proposed, gain] per word that has candidates -- proposed is the entry that replaces text[start:end],
       null for no proposal.  With --apply the line also holds the corrected text.

       Files are read, and given their contexts, as `score` does; the words are chosen as `words` chooses them.

       With --channel (what `confusions --counts` printed for OCR of the same kind) the look-up is the
       noisy-channel one: an entry costs what the learned confusions and --unit-bits per unexplained edit make
       of the way from it to the word, the candidates are the cheapest entries within --max-bits, and
       --channel-weight times these bits are added to the model's before the choice.

       With --boundaries a lost or spurious space is a hypothesis too (--max-dist counts it as one edit), and
       every record has a sixth field: "merge" for a span over two words and the space between them, "split"
       where the proposal puts a space into the word, "word" otherwise.  With --max-parts N a word may fall
       into up to N entries ("split" too).  With --compounds N a word that is no entry but a chain of 2 .. N
       entries, --links between them allowed, is left alone as an entry is.
    """
    from ..lib import windows
    rater = _load(model)
    more = {}
    if boundaries:
        more.update(boundaries=True, min_part=min_part, max_parts=max_parts)
    if compounds:
        if compounds < 2:
            raise click.UsageError("--compounds is 0 or 2 .. 8")
        more.update(compounds=compounds, min_part=min_part, links=tuple(s for s in (links or "").split(",") if s))
    try:
        lexicon = rater.lexicon(_read_lexicon(lexicon_file))
        if channel_file is not None:
            more.update(channel=rater.channel(_read_channel(channel_file), unit_bits=unit_bits, min_count=min_count,
                                                 min_rate=min_rate), max_bits=max_bits, channel_weight=channel_weight)
    except (ValueError, KeyError, TypeError) as err:
        raise click.UsageError(str(err))
    names, texts, contexts = [], [], []
    for file in _open_all(data):
        with file:
            texts.append(windows.normalize(file.read()))
        names.append(file.name)
        contexts.append(windows.context_from_filename(file.name))
    if not texts:
        return
    try:
        _, found, _ = rater.correct_words(texts, lexicon, contexts, max_dist=max_dist, per_word=per_word, known=known,
                                          delimiters=delimiters, k=k, max_prob=max_prob, min_rank=min_rank,
                                          min_suspects=min_suspects, min_bits_per_char=min_bits_per_char, min_chars=min_chars,
                                          left=left, ahead=ahead, min_gain=min_gain, streams=streams, precision=precision,
                                          **more)
    except ValueError as err:
        raise click.UsageError(str(err))
    for name, text, one in zip(names, texts, found):
        rows = [[int(a), int(b), text[int(a):int(b)], new, float(g)]
                for a, b, new, g in zip(one.starts, one.ends, one.proposals(), one.gain)]
        if boundaries:      # (a word holds no delimiter: a span with a space is a pair, a space in the proposal a split)
            rows = [row + ["merge" if " " in row[2] else "split" if row[3] is not None and " " in row[3] else "word"] for row in rows]
        line = {"file": name, "chars": len(text), "rescored": rows}
        if apply_:
            line["corrected"] = one.apply(text)
        click.echo(json.dumps(line, ensure_ascii=False))


@cli.command('witnesses', short_help='let the model choose between every file and other readings of it')
@click.option('-m', '--model', default="model.h5", show_default=True, help='model file', type=click.Path(dir_okay=False, exists=True))
@click.option('--witness', 'witness_dirs', multiple=True, required=True, type=click.Path(file_okay=False, exists=True),
              help='directory of second readings: the witness of a DATA file is the file of the same base name (may be missing); '
                   'repeat for further witnesses')
@click.option('--max-dist', default=32, show_default=True, type=click.IntRange(min=1, max=255),
              help='a witness further than this many edits from its file is not a reading of the same text')
@click.option('--join', default=1, show_default=True, type=click.IntRange(min=0),
              help='differences with at most this many equal characters between them are one span')
@click.option('-s', '--streams', default=1024, show_default=True, help='rows of a window call: hypotheses',
              type=click.IntRange(min=1, max=4096))
@click.option('--precision', default='bf16', show_default=True, type=click.Choice(['bf16', 'split']),
              help='bf16: bulk rating on the training forward; split: the inference kernels, ~f32 accuracy')
@click.option('--left', default=64, show_default=True, type=click.IntRange(min=1, max=1024),
              help='characters in front of a span that a hypothesis is read from (from a zero state)')
@click.option('--ahead', default=8, show_default=True, type=click.IntRange(min=0, max=1023),
              help='characters after a span that a hypothesis is held against')
@click.option('--min-gain', default=1.0, show_default=True, type=click.FLOAT,
              help='a proposal must save at least this many bits against the text as written')
@click.option('--apply', 'apply_', is_flag=True, default=False, help='also give the text with the proposals applied ("corrected")')
@click.argument('data', nargs=-1, type=click.Path(exists=True, dir_okay=True, file_okay=True))
def witnesses_(model, witness_dirs, max_dist, join, streams, precision, left, ahead, min_gain, apply_, data):
    """Align every DATA file with its witnesses -- the files of the same base name in the --witness
       directories --, rate the witnesses' readings of the spans where they differ against the text
       around them, and print one JSON line per file: characters, "witnesses": one {"file", "dist"} per
       witness found (dist -1: more than --max-dist edits apart, not used), "rescored" as `rescore` prints
       it, and "skipped": what yielded no hypothesis, by reason.  With --apply the line also holds the
       corrected text.  A file or witness of more than 4096 characters is an error: cut pages into lines.
    """
    from ..lib import ratebatch, windows
    rater = _load(model)
    names, texts, contexts, readings, sources = [], [], [], [], []
    for file in _open_all(data):
        with file:
            texts.append(windows.normalize(file.read()))
        names.append(file.name)
        contexts.append(windows.context_from_filename(file.name))
        paths = [os.path.join(d, os.path.basename(file.name)) for d in witness_dirs]
        sources.append([p for p in paths if os.path.isfile(p)])
        readings.append([])
        for path in sources[-1]:
            with open(path, mode='r') as other:
                readings[-1].append(windows.normalize(other.read()))
    if not texts:
        return
    try:
        alignments, found, _ = rater.merge_witnesses(texts, readings, contexts, max_dist=max_dist, join=join, left=left,
                                                     ahead=ahead, min_gain=min_gain, streams=streams, precision=precision)
    except ValueError as err:
        raise click.UsageError(str(err))
    for i, (name, text, one) in enumerate(zip(names, texts, found)):
        rows = [[int(a), int(b), text[int(a):int(b)], new, float(g)]
                for a, b, new, g in zip(one.starts, one.ends, one.proposals(), one.gain)]
        # (the counts of this file alone: witness_edits on its own alignments)
        _, skipped = ratebatch.witness_edits(alignments[i], [(0, w) for w in range(len(readings[i]))], [text], [readings[i]])
        line = {"file": name, "chars": len(text),
                "witnesses": [{"file": path, "dist": al.dist} for path, al in zip(sources[i], alignments[i])],
                "rescored": rows, "skipped": skipped}
        if apply_:
            line["corrected"] = one.apply(text)
        click.echo(json.dumps(line, ensure_ascii=False))


@cli.command('confusions', short_help='count the confusions of OCR files against their ground truth')
@click.option('-m', '--model', default="model.h5", show_default=True, help='model file', type=click.Path(dir_okay=False, exists=True))
@click.option('--truth', 'truth_dir', required=True, type=click.Path(file_okay=False, exists=True),
              help='directory of ground truth: the truth of a DATA file is the file of the same base name (a file without one is left out)')
@click.option('--max-dist', default=32, show_default=True, type=click.IntRange(min=1, max=255),
              help='a file further than this many edits from its truth is not a reading of it')
@click.option('--join', default=0, show_default=True, type=click.IntRange(min=0),
              help='differences with at most this many equal characters between them are one span')
@click.option('--max-chars', default=4, show_default=True, type=click.IntRange(min=1, max=4),
              help='characters of a source and of a replacement at most')
@click.option('--min-count', default=2, show_default=True, type=click.IntRange(min=0), help='a rule was seen at least this often')
@click.option('--min-rate', default=0.0, show_default=True, type=click.FLOAT,
              help='... and at no less than this share of the occurrences of its source')
@click.option('--per-source', default=3, show_default=True, type=click.IntRange(min=1), help='replacements of a source at most')
@click.option('--counts', is_flag=True, default=False,
              help='one JSON line per kept record (source, target, count, occ, rate) instead of the TSV')
@click.argument('data', nargs=-1, type=click.Path(exists=True, dir_okay=True, file_okay=True))
def confusions_(model, truth_dir, max_dist, join, max_chars, min_count, min_rate, per_source, counts, data):
    """Align every DATA file -- OCR output -- with its ground truth, the file of the same base name in
       --truth, count the differences and print the table of confusions: TSV lines of a source and its
       replacements, the most frequent first, as `rescore --confusions` reads them (an empty field drops the
       source).  With --counts one JSON line per kept record instead.  A last line on stderr gives the
       pairs, what was skipped (files further than --max-dist from their truth: "different"; spans of more
       than --max-chars characters: "long"; spans of an empty file: "empty"), the truth's characters, the
       edits and the character error rate.  A file of more than 4096 characters is an error: cut pages
       into lines.
    """
    from ..lib import windows
    rater = _load(model)
    texts, truths = [], []
    for file in _open_all(data):
        with file:
            text = windows.normalize(file.read())
        path = os.path.join(truth_dir, os.path.basename(file.name))
        if os.path.isfile(path):
            with open(path, mode='r') as other:
                truths.append(windows.normalize(other.read()))
            texts.append(text)
    try:
        found = rater.confusions(texts, truths, max_dist=max_dist, join=join, max_chars=max_chars)
    except ValueError as err:
        raise click.UsageError(str(err))
    same = dict(min_count=min_count, min_rate=min_rate, per_source=per_source)
    if counts:
        for rows in found.kept(**same):
            for i in rows:
                click.echo(json.dumps({"source": found.sources[i], "target": found.targets[i], "count": int(found.count[i]),
                                       "occ": int(found.occ[i]), "rate": found.rate(i)}, ensure_ascii=False))
    else:
        found.write(click.get_text_stream('stdout'), **same)
    click.echo(json.dumps(dict(found.skipped, pairs=len(texts), chars=found.chars, edits=found.edits, cer=found.cer)), err=True)


@cli.command('consensus', short_help='let the model and the votes choose among several readings of every file')
@click.option('-m', '--model', default="model.h5", show_default=True, help='model file', type=click.Path(dir_okay=False, exists=True))
@click.option('--witness', 'witness_dirs', multiple=True, required=True, type=click.Path(file_okay=False, exists=True),
              help='directory of second readings: the witness of a DATA file is the file of the same base name (may be missing); '
                   'repeat for further witnesses, at most 64')
@click.option('--max-dist', default=32, show_default=True, type=click.IntRange(min=1, max=255),
              help='a witness further than this many edits from its file is not a reading of the same text')
@click.option('--join', default=1, show_default=True, type=click.IntRange(min=0),
              help='differences of any witnesses with at most this many equal characters between them are one span')
@click.option('--vote-bits', default=0.0, show_default=True, type=click.FloatRange(min=0.0),
              help='bits a reading is credited per witness that gives it (the text as written: itself and every witness that agrees); '
                   '0: the model alone')
@click.option('-s', '--streams', default=1024, show_default=True, help='rows of a window call: hypotheses',
              type=click.IntRange(min=1, max=4096))
@click.option('--precision', default='bf16', show_default=True, type=click.Choice(['bf16', 'split']),
              help='bf16: bulk rating on the training forward; split: the inference kernels, ~f32 accuracy')
@click.option('--left', default=64, show_default=True, type=click.IntRange(min=1, max=1024),
              help='characters in front of a span that a hypothesis is read from (from a zero state)')
@click.option('--ahead', default=8, show_default=True, type=click.IntRange(min=0, max=1023),
              help='characters after a span that a hypothesis is held against')
@click.option('--min-gain', default=1.0, show_default=True, type=click.FLOAT,
              help='a proposal must score at least this many bits better than the text as written')
@click.option('--apply', 'apply_', is_flag=True, default=False, help='also give the text with the proposals applied ("corrected")')
@click.argument('data', nargs=-1, type=click.Path(exists=True, dir_okay=True, file_okay=True))
def consensus_(model, witness_dirs, max_dist, join, vote_bits, streams, precision, left, ahead, min_gain, apply_, data):
    """Align every DATA file with its witnesses -- the files of the same base name in the --witness
       directories --, cluster the differences of all witnesses of a file, rate every distinct reading
       of a cluster against the text around it, and print one JSON line per file as `witnesses` does:
       characters, "witnesses": one {"file", "dist"} per witness found, and "rescored": per cluster
       [start, end, written, proposal, gain, votes of the text as written, [[reading, votes], ...]].
       With --apply the line also holds the corrected text.  A last line on stderr gives what yielded no
       hypothesis, by reason.  A file or witness of more than 4096 characters is an error: cut pages
       into lines.
    """
    from ..lib import windows
    rater = _load(model)
    names, texts, contexts, readings, sources = [], [], [], [], []
    for file in _open_all(data):
        with file:
            texts.append(windows.normalize(file.read()))
        names.append(file.name)
        contexts.append(windows.context_from_filename(file.name))
        paths = [os.path.join(d, os.path.basename(file.name)) for d in witness_dirs]
        sources.append([p for p in paths if os.path.isfile(p)])
        readings.append([])
        for path in sources[-1]:
            with open(path, mode='r') as other:
                readings[-1].append(windows.normalize(other.read()))
    if not texts:
        return
    try:
        found, dists, skipped = rater.consensus(texts, readings, contexts, max_dist=max_dist, join=join, vote_bits=vote_bits,
                                                left=left, ahead=ahead, min_gain=min_gain, streams=streams, precision=precision,
                                                want_costs=False)
    except ValueError as err:
        raise click.UsageError(str(err))
    for i, (name, text, one) in enumerate(zip(names, texts, found)):
        first = one.first.tolist()
        rows = [[int(a), int(b), text[int(a):int(b)], new, float(g), int(v0),
                 [[c, int(v)] for c, v in zip(one.candidates[first[j]:first[j + 1]], one.votes[first[j]:first[j + 1]])]]
                for j, (a, b, new, g, v0) in enumerate(zip(one.starts, one.ends, one.proposals(), one.gain, one.votes0))]
        line = {"file": name, "chars": len(text),
                "witnesses": [{"file": path, "dist": int(d)} for path, d in zip(sources[i], dists[i])], "rescored": rows}
        if apply_:
            line["corrected"] = one.apply(text)
        click.echo(json.dumps(line, ensure_ascii=False))
    click.echo(json.dumps(skipped), err=True)


@cli.command(short_help='sample characters from language model')
@click.option('-m', '--model', required=True, help='model file', type=click.Path(dir_okay=False, exists=True))
@click.option('-n', '--number', default=1, help='number of characters to sample', type=click.IntRange(min=1, max=10000))
@click.option('-v', '--variants', default=1, help='number of character sequences to sample',
              type=click.IntRange(min=1, max=10000))
@click.option('-c', '--context', default=None, help='constant meta-data input')
@click.option('--device-beam', is_flag=True, default=False,
              help='expand and prune the beam on the GPU, all characters enqueued without a wait (Rater.device_beam)')
@click.option('--sample', is_flag=True, default=False,
              help='draw the sequences from the model\'s distribution (Rater.sample) instead of searching for the most probable ones')
@click.option('--temperature', default=1.0, show_default=True, type=click.FloatRange(min=0.0),
              help='with --sample: below 1 sharpens the distribution, 0 always takes the most probable character')
@click.option('--top-k', default=0, show_default=True, type=click.IntRange(min=0, max=64),
              help='with --sample: draw among the K most probable characters only (0: all)')
@click.option('--seed', default=0, show_default=True, type=click.IntRange(min=0),
              help='with --sample: the same seed draws the same sequences')
@click.argument('prefix', type=click.STRING)
def generate(model, number, variants, context, device_beam, sample, temperature, top_k, seed, prefix):
    """Apply a language model, generating the most probable characters (starting with PREFIX string).

       With --sample the VARIANTS sequences are drawn at random from the model's distribution instead.
    """
    rater = _load(model, incremental=True)
    if device_beam:
        rater.device_beam = True
    ctx = _contexts(context) if context else rater.underspecify_contexts()
    if sample:
        results = rater.sample(prefix, number, ctx, variants, temperature=temperature, top_k=top_k, seed=seed)
    else:
        results = rater.generate(prefix, number, ctx, variants)
    for res in results:
        click.echo(prefix[:-1] + res)


@cli.command(short_help='Print the training history')
@click.option('-m', '--model', required=True, help='model file', type=click.Path(dir_okay=False, exists=True))
def print_history(model):
    rater = lib.Rater()
    rater.load_config(model)
    rater.print_history()


@cli.command(short_help='Print the mapped characters')
@click.option('-m', '--model', required=True, help='model file', type=click.Path(dir_okay=False, exists=True))
def print_charset(model):
    rater = lib.Rater()
    rater.load_config(model)
    rater.print_charset()


@cli.command(short_help='Delete one character from mapping')
@click.option('-m', '--model', required=True, help='model file', type=click.Path(dir_okay=False, exists=True, writable=True))
@click.argument('char')
def prune_charset(model, char):
    rater = _load(model)
    if rater.remove_from_mapping(char=char):
        rater.save(model)


@cli.command(short_help='Paint a heat map of character embeddings')
@click.option('-m', '--model', required=True, help='model file', type=click.Path(dir_okay=False, exists=True))
@click.argument('filename', type=click.Path(dir_okay=False, writable=True))
def plot_char_embeddings_similarity(model, filename):
    _load(model).plot_char_embeddings_similarity(filename)


@cli.command(short_help='Paint a heat map of context embeddings')
@click.option('-m', '--model', required=True, help='model file', type=click.Path(dir_okay=False, exists=True))
@click.option('-n', '--number', default=1, help='which context variable', type=click.IntRange(min=1, max=100))
@click.argument('filename', type=click.Path(dir_okay=False, writable=True))
def plot_context_embeddings_similarity(model, filename, number):
    _load(model).plot_context_embeddings_similarity(filename, n=number)


@cli.command(short_help='Paint a 2-d PCA projection of context embeddings')
@click.option('-m', '--model', required=True, help='model file', type=click.Path(dir_okay=False, exists=True))
@click.option('-n', '--number', default=1, help='which context variable', type=click.IntRange(min=1, max=100))
@click.argument('filename', type=click.Path(dir_okay=False, writable=True))
def plot_context_embeddings_projection(model, filename, number):
    _load(model).plot_context_embeddings_projection(filename, n=number)


if __name__ == '__main__':
    cli()
