"""Ship slices of the two wide-observation datasets of the reference as committed fixtures (DATA only: observation and
latent-state arrays copied from its pickles, float32: the path computes in fp32).

    python tests/golden/make_wobs_slices.py          (build container: reads /root/reference, numpy pickles)

Sources
  * /root/reference/data/lorenz/lorenzdatadict_py3 -- Lorenz attractor, Dx = 3, Dy = 10: Ytrain (66, 250, 10),
    Yvalid (17, 250, 10), Ytest (17, 250, 10), State (100, 250, 3) (the latent trajectories of all 100 sequences: rows 0..65
    belong to Ytrain, 66..82 to Yvalid, 83..99 to Ytest).
  * /root/reference/data/vind/datadict -- Dx = 2, Dy = 20: Ytrain (80, 30, 20), Yvalid (10, 30, 20), Xtrain (80, 30, 2),
    Xvalid (10, 30, 2).

Written
  tests/golden/lorenz_slice.npz   Ytrain (8, 100, 10) = Ytrain[:8, :100], Yvalid (4, 100, 10) = Yvalid[:4, :100],
                                  State_train (8, 100, 3) = State[:8, :100], State_valid (4, 100, 3) = State[66:70, :100]
  tests/golden/vind_slice.npz     Ytrain (8, 30, 20), Yvalid (4, 30, 20), Xtrain (8, 30, 2), Xvalid (4, 30, 2)
Consumers: tests/test_wobs_host.py (shapes), tests/test_gpu_wobs.py (runner.main on each slice)."""
import os
import pickle

import numpy as np

LORENZ = "/root/reference/data/lorenz/lorenzdatadict_py3"
VIND = "/root/reference/data/vind/datadict"
HERE = os.path.dirname(os.path.abspath(__file__))


def _load(path):
    with open(path, "rb") as f:
        try:
            return pickle.load(f)
        except UnicodeDecodeError:
            f.seek(0)
            return pickle.load(f, encoding="latin1")


def _save(name, **arrays):
    dst = os.path.join(HERE, name)
    np.savez_compressed(dst, **{k: np.ascontiguousarray(v, dtype=np.float32) for k, v in arrays.items()})
    print(dst, os.path.getsize(dst), {k: v.shape for k, v in arrays.items()})


if __name__ == "__main__":
    d = _load(LORENZ)
    n_train = d["Ytrain"].shape[0]
    assert d["Ytrain"].shape == (66, 250, 10) and d["State"].shape == (100, 250, 3)
    _save("lorenz_slice.npz", Ytrain=d["Ytrain"][:8, :100], Yvalid=d["Yvalid"][:4, :100],
          State_train=d["State"][:8, :100], State_valid=d["State"][n_train:n_train + 4, :100])
    d = _load(VIND)
    assert d["Ytrain"].shape == (80, 30, 20) and d["Xtrain"].shape == (80, 30, 2)
    _save("vind_slice.npz", Ytrain=d["Ytrain"][:8], Yvalid=d["Yvalid"][:4], Xtrain=d["Xtrain"][:8], Xvalid=d["Xvalid"][:4])
