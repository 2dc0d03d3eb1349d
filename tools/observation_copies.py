"""python tools/observation_copies.py -- device-event times of the two per-update observation copies at config 3's shape (32 workers x 512 steps x 3 x 84 x 84), float32 and uint8:
staging [S, W, ...] -> buffer [W, S, ...] (trainer._finish_rollout) and buffer -> NHWC (trainer._observations_channels_last)."""
import torch
dev = torch.device("cuda", 0)
S, W = 512, 32
for dt in (torch.float32, torch.uint8):
    stage = torch.zeros((S, W, 3, 84, 84), dtype=dt, device=dev)
    buf = torch.zeros((W, S, 3, 84, 84), dtype=dt, device=dev)
    nhwc = torch.empty((W * S, 84, 84, 3), dtype=dt, device=dev)
    flat = buf.reshape(W * S, 3, 84, 84)
    for name, fn in (("staging -> buffer", lambda: buf.copy_(stage.transpose(0, 1))), ("buffer -> NHWC", lambda: nhwc.copy_(flat.permute(0, 2, 3, 1)))):
        ts = []
        for i in range(12):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        ts = sorted(ts[2:])
        nbytes = stage.numel() * stage.element_size()
        print(f"{str(dt):14s} {name:18s} median {ts[len(ts) // 2] * 1e3:8.1f} us  (min {ts[0] * 1e3:.1f}, max {ts[-1] * 1e3:.1f}; {nbytes / 1e9:.3f} GB read + as much written: "
              f"{2 * nbytes / (ts[len(ts) // 2] * 1e-3) / 1e12:.2f} TB/s)")
    del stage, buf, nhwc, flat
