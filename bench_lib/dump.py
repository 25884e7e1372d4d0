"""bench.py --dump-outputs: what the timed loop hands its caller after a step, as float32 / float64 .npy files."""
import os

import numpy as np

DUMP_BYTES = 64 * 10**6          # everything written, .npy headers included
SAMPLE_SEED = 0x0B5              # the envs whose frames are written when the frames of all of them would not fit


def write_outputs(sim, results, out_dir):
    """reward, game_over code and action of every env (float32), the frames of a fixed, seeded sample of envs (float32, pixel
    values as stored: 0..255 for uint8 frames) and that sample's env indices (float64).  Returns {name: shape}.
    results: the [num_envs, 2] (reward, game_over code) row the step wrote into the results ring -- the codes the step
    computed: reset_done clears those of the finished envs in the batch's own buffer."""
    import torch
    n = sim.num_envs
    results = results.cpu().numpy()
    arrays = {"reward": results[:, 0].astype(np.float32),
              "game_over": results[:, 1].astype(np.float32),
              "actions": sim.actions.cpu().numpy().astype(np.float32)}
    obs = sim.obs
    room = DUMP_BYTES - (1 << 16) - sum(a.nbytes for a in arrays.values()) - 8 * n
    m = min(n, room // (obs[0].numel() * 4))
    assert m > 0, "one env's frames exceed the dump's size limit"
    envs = np.arange(n) if m == n else np.sort(np.random.default_rng(SAMPLE_SEED).choice(n, size=m, replace=False))
    arrays["obs"] = obs[torch.as_tensor(envs, device=obs.device)].float().cpu().numpy()
    arrays["obs_envs"] = envs.astype(np.float64)
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return {name: list(a.shape) for name, a in arrays.items()}
