"""Writes tests/golden/hubert_small.npz: transformers' own HubertModel outputs for the small test configuration (development container only:
needs `transformers`; offline, random weights, nothing is downloaded).  No test needs transformers at run time.

The state dict and the waves are NOT stored as arrays (2 MB and 2.6 MB, above the size limit of a committed file): the fixture holds their
seeds, and tests/hubert_ref.py's make_state_dict / make_wave regenerate them bit for bit (torch's CPU generator).  Stored:
  sd_seed, wave_seeds, wave_lens                     the seeded inputs
  sd_checksum, wave_checksums                        float64 sums of |values|, so that a changed generator is noticed
  out32_<n>, out64_<n>   n = 400, 719, 720, 16000    last_hidden_state of HubertModel in float32 / float64
  long_rows, long64                                  the chunked result (get_hubert_from_16k_speech_long's rule, float64 model) of the
                                                     2 x 320000 + 5000 sample wave at the rows long_rows: the first and last 8, 24 rows around
                                                     each chunk seam and every 16th row (all 2015 rows would be 2 MB)
  long_num_rows                                      its full row count
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hubert_ref  # noqa: E402

SD_SEED = 20240
SHORT = (400, 719, 720, 16000)
LONG = 2 * 320000 + 5000


def long_rows(total):
    rows = set(range(8)) | set(range(total - 8, total)) | set(range(0, total, 16))
    for seam in (1000, 2000):
        rows |= set(range(seam - 12, min(seam + 12, total)))
    return np.array(sorted(rows), dtype=np.int64)


def main():
    from transformers import HubertConfig, HubertModel
    c = hubert_ref.SMALL
    cfg = HubertConfig(hidden_size=c["hidden"], num_hidden_layers=c["layers"], num_attention_heads=c["heads"], intermediate_size=c["intermediate"],
                       conv_dim=list(c["conv_dim"]), conv_kernel=list(c["conv_kernel"]), conv_stride=list(c["conv_stride"]),
                       num_conv_pos_embeddings=c["pos_kernel"], num_conv_pos_embedding_groups=c["pos_groups"], layer_norm_eps=c["ln_eps"],
                       feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True, feat_proj_layer_norm=True, hidden_act="gelu",
                       feat_extract_activation="gelu")
    model = HubertModel(cfg).eval()
    sd = hubert_ref.make_state_dict(c, SD_SEED)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and set(missing) <= {"masked_spec_embed"}, (missing, unexpected)
    out = {"sd_seed": SD_SEED, "sd_checksum": sum(float(v.double().abs().sum()) for v in sd.values()),
           "wave_lens": np.array(SHORT + (LONG,)), "wave_seeds": np.array([100 + i for i in range(len(SHORT) + 1)])}
    sums = []
    with torch.no_grad():
        for i, n in enumerate(SHORT):
            w = hubert_ref.make_wave(n, 100 + i)
            sums.append(float(w.double().abs().sum()))
            out[f"out32_{n}"] = model.float()(w[None]).last_hidden_state[0].numpy()
            out[f"out64_{n}"] = model.double()(w.double()[None]).last_hidden_state[0].numpy()
        w = hubert_ref.make_wave(LONG, 100 + len(SHORT))
        sums.append(float(w.double().abs().sum()))
        model.double()
        full = hubert_ref.chunked(lambda x: model(x).last_hidden_state, w.double())
        rows = long_rows(full.shape[0])
        out["long_num_rows"] = full.shape[0]
        out["long_rows"] = rows
        out["long64"] = full[rows].numpy()
    out["wave_checksums"] = np.array(sums)
    path = os.path.join(HERE, "hubert_small.npz")
    np.savez(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
