"""bench.py --dump-outputs DIR: what the timed path computed in its last step, as .npy files, so that two builds can be compared output
for output.  The path's outputs are the int32 score and the int32 (x, y) sink of every alignment; a batch larger than MAX_ROWS is written
as a fixed, seeded sample of MAX_ROWS alignments (the same rows in every run).  float64 holds every int32 exactly.

  DIR/index.npy  float64 [m]     the alignments written (ascending job indices)
  DIR/score.npy  float64 [m]     their scores
  DIR/sink.npy   float64 [m, 2]  their sinks

At MAX_ROWS = 2^20 that is 32 MB in all."""
import os

import numpy as np
import torch

MAX_ROWS = 1 << 20
SAMPLE_SEED = 0x5EED0005


def sample_index(n, max_rows=MAX_ROWS, seed=SAMPLE_SEED):
    """the job indices written for a batch of n: all of them up to max_rows, else a seeded sample of max_rows, ascending"""
    if n <= max_rows:
        return np.arange(n, dtype=np.int64)
    return np.sort(np.random.Generator(np.random.PCG64(seed)).choice(n, max_rows, replace=False)).astype(np.int64)


def write_outputs(d, score, sink, max_rows=MAX_ROWS):
    """score: int32 [n], sink: int32 [n, 2] (device or host tensors) -> DIR/{index,score,sink}.npy; returns the paths"""
    os.makedirs(d, exist_ok=True)
    idx = sample_index(score.shape[0], max_rows)
    it = torch.from_numpy(idx).to(score.device)
    arrays = {"index": idx.astype(np.float64),
              "score": score[it].cpu().numpy().astype(np.float64),
              "sink": sink[it].cpu().numpy().astype(np.float64)}
    paths = []
    for name, arr in arrays.items():
        p = os.path.join(d, name + ".npy")
        np.save(p, arr)
        paths.append(p)
    return paths
