#!/usr/bin/env python3
"""Drop-in for the reference's train-model.py on the MI355X path: same constants, same loop semantics
(music-style-transfer_amd/style/train.py), run from the repository root:

    python train-model.py [--batch-clips K [--window-bars R] [--store-songs N] [--window-seed S] [--eval-windows M]
                           [--refresh-every E [--refresh-songs M] [--store-records R]]] [data_path] [n_eval_files [eval_every]]

With n_eval_files > 0 the last that many of the sorted files are held out of training and evaluated (forward, loss and note
metrics, no backward) after every eval_every-th iteration (default 100) into validation.csv.
With --batch-clips K the loop trains on windowed batches (style.train.train's batch_clips, window_bars, store_songs,
window_seed): N songs are kept on the device and every iteration is one batched pass over K windows of R bars of them.
With --eval-windows M as well (and n_eval_files > 0) validation follows: M held-out songs are kept on the device and every
evaluation round scores the same fixed windows of R bars of them in batches of K (style.train.evaluate_windows).
With --refresh-every E the N songs are a fixed ring on the device (of --store-records R note records per pool; default: twice
what the first N songs need): after every E-th iteration the next --refresh-songs M songs of the data (default 4) come in and
the oldest leave, so the batched loop walks through the whole data set in fixed device memory.
"""
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, 'music-style-transfer_amd'))

from style.train import main  # noqa: E402

WINDOW_OPTIONS = {'--batch-clips': 'batch_clips', '--window-bars': 'window_bars', '--store-songs': 'store_songs',
                  '--window-seed': 'window_seed', '--eval-windows': 'eval_windows', '--refresh-every': 'refresh_every',
                  '--refresh-songs': 'refresh_songs', '--store-records': 'store_records'}


def split_options(argv):
    """(positional arguments, the windowed-batch options as keyword arguments of style.train.train)."""
    positional, options = [], {}
    argv = list(argv)
    while argv:
        arg = argv.pop(0)
        if arg in WINDOW_OPTIONS:
            if not argv:
                raise SystemExit(f'{arg} needs a value')
            options[WINDOW_OPTIONS[arg]] = int(argv.pop(0))
        else:
            positional.append(arg)
    if options and 'batch_clips' not in options:
        raise SystemExit('--window-bars, --store-songs, --window-seed and --eval-windows go with --batch-clips')
    if ('refresh_songs' in options or 'store_records' in options) and 'refresh_every' not in options:
        raise SystemExit('--refresh-songs and --store-records go with --refresh-every')
    return positional, options


if __name__ == '__main__':
    args, windows = split_options(sys.argv[1:])
    n_eval_files = int(args[1]) if len(args) > 1 else 0
    held_out = dict(n_eval_files=n_eval_files, eval_every=int(args[2]) if len(args) > 2 else 100) if n_eval_files else {}
    kwargs = dict(n_iterations=5000, iter_size=2, training_info_path='training.csv', save_path='snapshots/', save_interval=100)
    kwargs.update(held_out)
    if windows:
        kwargs.update(windows, iter_size=1)      # K clips accumulate per optimizer step: K takes iter_size's place
    main(*(args[:1] or ['data/Lakh MIDI Dataset/clean_midi/']), **kwargs)
