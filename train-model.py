#!/usr/bin/env python3
"""Drop-in for the reference's train-model.py on the MI355X path: same constants, same loop semantics
(music-style-transfer_amd/style/train.py), run from the repository root:

    python train-model.py [data_path] [n_eval_files [eval_every]]

With n_eval_files > 0 the last that many of the sorted files are held out of training and evaluated (forward, loss and note
metrics, no backward) after every eval_every-th iteration (default 100) into validation.csv.
"""
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, 'music-style-transfer_amd'))

from style.train import main  # noqa: E402

if __name__ == '__main__':
    n_eval_files = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    held_out = dict(n_eval_files=n_eval_files, eval_every=int(sys.argv[3]) if len(sys.argv) > 3 else 100) if n_eval_files else {}
    main(*(sys.argv[1:2] or ['data/Lakh MIDI Dataset/clean_midi/']), n_iterations=5000, iter_size=2,
         training_info_path='training.csv', save_path='snapshots/', save_interval=100, **held_out)
