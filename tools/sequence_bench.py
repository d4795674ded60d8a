"""Frame-sequence timing: one sequence.eval against the loop a user writes without it.

Workload: RGB, FAST, n = 2^21 upper-hemisphere directions, K in {24, 365} frames (hourly suns
of one day; one daylight sun per day of a year), each frame with its own turbidity and weight.
  baseline -- K x (set sun_direction and turbidity, parameters_changed_async, eval,
              out.add_(tmp, alpha=w)) on one stream
  sequence -- one SunskySequence.eval
time.perf_counter around stream-synchronised bursts, warm, median of 5.  Prints one JSON line
per K: both times, their ratio, and the sequence kernel's frame-evals/s (n K / t: a frame-eval
does an eval's transcendental work with no HBM traffic).  Not part of bench.py.
  --sampling -- instead: sample_direction and pdf_direction of the prepared sequence beside
                sequence.eval at the sampled directions (see sampling()).
  --grad     -- instead: sequence.eval_vjp beside sequence.eval in reference precision and the
                per-frame loop it replaces (see grad(); --no-loop leaves the loop out, for a
                profiler run of the sequence kernels alone).
  --irradiance -- instead: sequence.irradiance on 2^20 receivers beside the chunked torch
                formulation a user writes from the read-back tables (see irradiance()).
  --irradiance-grad -- instead: sequence.irradiance_vjp beside sequence.irradiance and the torch
                formulations of both gradients (see irradiance_grad()).
  --irradiance-horizon-grad -- instead: sequence.irradiance_vjp(horizon=...) beside the open
                irradiance_vjp, irradiance(horizon=...) and torch autograd through the masked
                formulation (see irradiance_horizon_grad()).
  --irradiance-horizon -- instead: sequence.irradiance under a shared and a per-receiver horizon
                profile beside the unoccluded call and the masked chunked torch formulation
                (see irradiance_horizon()).
  --irradiance-series -- instead: sequence.irradiance_series, every frame's own irradiance in one
                call, beside K one-frame sequences' irradiance calls (see irradiance_series())."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "mitsuba3-sunsky_amd"))
import sunsky_amd as ss  # noqa: E402

N = 1 << 21
REPS = 5


def frames(k):
    if k == 24:
        times = [(2010, 7, 10, float(h)) for h in range(24)]
    else:
        times = [(2010, 1 + (d * 12) // k, 1 + d % 28, 8.0 + (d % 9)) for d in range(k)]
    dirs = np.stack([ss.sun_coordinates(*t) for t in times]).astype(np.float32)
    turb = (1.0 + 9.0 * ((7 * np.arange(k)) % k) / max(k - 1, 1)).astype(np.float32)
    wts = (0.25 + ((5 * np.arange(k)) % 11) / 8.0).astype(np.float32)
    return dirs, turb, wts


def median_ms(step, reps=REPS):
    step()                      # warm
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), ts


def sampling(ks, dev):
    """--sampling: sample_direction and pdf_direction of a prepared sequence (64 x 256 table)
    beside sequence.eval of the same n and K in the same session: the fused sampler runs eval's
    frame loop plus a prologue, so eval is its yardstick.  pdf_direction walks one 16-byte
    record per frame: reported as frame x directions / s."""
    g = torch.Generator(device=dev).manual_seed(3)
    u = torch.rand((2, N), device=dev, generator=g)
    base = {"type": "sunsky", "sun_direction": [0.3, 0.4, 0.866], "turbidity": 3.0, "albedo": 0.2}
    for k in ks:
        dirs, turb, wts = frames(k)
        seq = ss.SunskySequence(ss.load_dict(dict(base)), dirs, turb, wts)
        t0 = time.perf_counter()
        seq.prepare_sampling()
        t_prep = (time.perf_counter() - t0) * 1e3
        ds, _ = seq.sample_direction(None, u)
        wi = (-ds.d).contiguous()
        out = torch.empty((3, N), device=dev)
        t_eval, all_eval = median_ms(lambda: seq.eval(wi, out=out))
        t_samp, all_samp = median_ms(lambda: seq.sample_direction(None, u))
        t_pdf, all_pdf = median_ms(lambda: seq.pdf_direction(None, ds))
        info = seq.sampling_info()
        print(json.dumps({"K": k, "n": N, "table": [info["n_z"], info["n_phi"]], "w_sky": round(info["w_sky"], 4),
                          "prepare_ms": round(t_prep, 3), "eval_ms": round(t_eval, 3),
                          "sample_direction_ms": round(t_samp, 3), "sample_over_eval": round(t_samp / t_eval, 3),
                          "pdf_direction_ms": round(t_pdf, 3),
                          "pdf_frame_directions_per_s": round(N * k / (t_pdf * 1e-3), 0),
                          "eval_ms_all": [round(t, 3) for t in all_eval],
                          "sample_direction_ms_all": [round(t, 3) for t in all_samp],
                          "pdf_direction_ms_all": [round(t, 3) for t in all_pdf]}), flush=True)
    print("sequence_bench sampling done")


def grad(ks, dev, with_loop):
    """--grad: the reverse-mode gradient of a K-frame sequence (weights, turbidities, sun
    directions: 5 K values) for a normal cotangent, against two yardsticks of the same session:
    sequence.eval in reference precision at the same n and K (the gradient runs reference
    arithmetic), and the loop a user writes without it, K x (set sun_direction and turbidity,
    parameters_changed, eval_vjp for dT and ds, eval + a dot product for dw) on one stream."""
    g = torch.Generator(device=dev).manual_seed(3)
    v = torch.randn((3, N), device=dev, generator=g)
    v[2] = v[2].abs()
    wi = -(v / v.norm(dim=0, keepdim=True)).contiguous()
    si = ss.SurfaceInteraction3f(wi=wi)
    d_out = torch.randn((3, N), device=dev, generator=g)
    base = {"type": "sunsky", "sun_direction": [0.3, 0.4, 0.866], "turbidity": 3.0, "albedo": 0.2}
    for k in ks:
        dirs, turb, wts = frames(k)
        seq = ss.SunskySequence(ss.load_dict(dict(base)), dirs, turb, wts)
        seq.set_precision("reference")
        t0 = time.perf_counter()
        seq.prepare_grad()
        t_prep = (time.perf_counter() - t0) * 1e3
        out = torch.empty((3, N), device=dev)
        gr = {"weights": torch.zeros(k, device=dev), "turbidity": torch.zeros(k, device=dev),
              "sun_directions": torch.zeros((k, 3), device=dev)}
        t_eval, all_eval = median_ms(lambda: seq.eval(wi, out=out))
        t_vjp, all_vjp = median_ms(lambda: seq.eval_vjp(wi, d_out, grad=gr))
        line = {"K": k, "n": N, "prepare_grad_ms": round(t_prep, 3), "eval_reference_ms": round(t_eval, 3),
                "eval_vjp_ms": round(t_vjp, 3), "vjp_over_eval": round(t_vjp / t_eval, 3),
                "frame_grads_per_s": round(N * k / (t_vjp * 1e-3), 0),
                "eval_reference_ms_all": [round(t, 3) for t in all_eval], "eval_vjp_ms_all": [round(t, 3) for t in all_vjp]}
        if with_loop:
            em = ss.load_dict(dict(base))
            em.set_precision("reference")
            params = em.traverse()
            gw = torch.zeros(k, device=dev)
            g16 = torch.zeros((k, 16), device=dev)

            def loop():
                g16.zero_()
                for i in range(k):
                    params["sun_direction"] = dirs[i]
                    params["turbidity"] = float(turb[i])
                    params.update()
                    em.eval_vjp(si, d_out, grad=g16[i])
                    gw[i] = (em.eval(si) * d_out).sum()

            t_loop, all_loop = median_ms(loop)
            # Agreement of the two paths, away from the discs: set_param stages a sun direction as
            # given while a sequence normalises it, so a few disc-edge lanes sit on different sides
            # of the fp32 disc test (see main()), and a disc lane is ~1e5 x a sky lane in these
            # signed sums.  Lanes within two half apertures of any frame's sun are masked out of
            # both paths for this comparison only (the timings above are unmasked).  The loop's dT
            # is per unit weight.
            cut = float(np.cos(2.0 * em.info()["sun_half_aperture"]))
            keep = torch.ones(N, dtype=torch.bool, device=dev)
            for i in range(k):
                s = torch.from_numpy(dirs[i] / np.linalg.norm(dirs[i])).to(dev)
                keep &= (-(s[:, None] * wi).sum(0)) < cut
            mask = keep.to(torch.uint8)
            for key in gr:
                gr[key].zero_()
            seq.eval_vjp(wi, d_out, active=mask, grad=gr)
            g16.zero_()
            for i in range(k):
                params["sun_direction"] = dirs[i]
                params["turbidity"] = float(turb[i])
                params.update()
                em.eval_vjp(si, d_out, active=mask, grad=g16[i])
                gw[i] = (em.eval(si, mask) * d_out).sum()
            w_t = torch.from_numpy(wts).to(dev)
            scale = lambda a: a.abs().max().clamp_min(1e-30)  # noqa: E731
            line.update({"loop_ms": round(t_loop, 3), "speedup": round(t_loop / t_vjp, 2),
                         "loop_ms_all": [round(t, 3) for t in all_loop],
                         "lanes_compared": int(keep.sum().item()),
                         "max_diff_weights": float(((gr["weights"] - gw).abs() / scale(gw)).max()),
                         "max_diff_turbidity": float(((gr["turbidity"] - w_t * g16[:, 0]).abs() / scale(w_t * g16[:, 0])).max())})
        print(json.dumps(line), flush=True)
    print("sequence_bench grad done")


def irradiance(ks, dev):
    """--irradiance: E on n = 2^20 receivers with normals uniform on the sphere, RGB, 64 x 256
    cells.  The yardstick of the same session is what a user writes today from the tables read
    back once: relu(N_l D^T) @ (omega R)^T plus the sun term in torch, in chunks of 2^14 receivers
    (an n x cells intermediate per chunk).  Prints both medians, their ratio, receiver-cell pairs
    per second, prepare_irradiance's time and the largest difference of the two results."""
    n, chunk = 1 << 20, 1 << 14
    g = torch.Generator(device=dev).manual_seed(3)
    v = torch.randn((3, n), device=dev, generator=g)
    nrm = (v / v.norm(dim=0, keepdim=True)).contiguous()
    base = {"type": "sunsky", "sun_direction": [0.3, 0.4, 0.866], "turbidity": 3.0, "albedo": 0.2}
    for k in ks:
        dirs, turb, wts = frames(k)
        seq = ss.SunskySequence(ss.load_dict(dict(base)), dirs, turb, wts)
        seq.prepare_irradiance()    # warm: module load, allocator
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        seq.prepare_irradiance()
        t_prep = (time.perf_counter() - t0) * 1e3
        info = seq.irradiance_info()
        nz, nphi = info["n_z"], info["n_phi"]
        # the tables read back once, as device tensors (an identity to_world: N_l = N)
        z = (np.arange(nz) + 0.5) / nz
        phi = (np.arange(nphi) + 0.5) * (2 * np.pi / nphi)
        st = np.sqrt(1 - z * z)
        D = np.stack([np.outer(st, np.cos(phi)).ravel(), np.outer(st, np.sin(phi)).ravel(), np.repeat(z, nphi)], 1)
        D_t = torch.from_numpy(D.astype(np.float32)).to(dev)                                        # (cells, 3)
        R_t = torch.from_numpy(info["omega"] * seq.irradiance_table("sky").reshape(3, -1)).to(dev)   # (3, cells)
        S_t = torch.from_numpy(np.stack([seq.frame(i)["sun_dir_local"] for i in range(k)])).to(dev)  # (K, 3)
        F_t = torch.from_numpy(wts[None, :] * seq.irradiance_table("sun_flux")).to(dev)              # (3, K)
        out_t = torch.empty((3, n), device=dev)
        out = torch.empty((3, n), device=dev)

        def torch_chunks():
            for a in range(0, n, chunk):
                nl = nrm[:, a:a + chunk].t()
                e = torch.relu(nl @ D_t.t()) @ R_t.t() + torch.relu(nl @ S_t.t()) @ F_t.t()
                out_t[:, a:a + chunk] = e.t()

        t_kernel, all_kernel = median_ms(lambda: seq.irradiance(nrm, out=out))
        t_torch, all_torch = median_ms(torch_chunks)
        diff = float(((out - out_t).abs().max() / out_t.abs().max()).item())
        print(json.dumps({"K": k, "n": n, "table": [nz, nphi], "prepare_irradiance_ms": round(t_prep, 3),
                          "irradiance_ms": round(t_kernel, 3), "torch_chunked_ms": round(t_torch, 3),
                          "torch_over_kernel": round(t_torch / t_kernel, 2),
                          "receiver_cell_pairs_per_s": round(n * nz * nphi / (t_kernel * 1e-3), 0),
                          "max_diff_vs_torch_of_max": diff,
                          "irradiance_ms_all": [round(t, 3) for t in all_kernel],
                          "torch_chunked_ms_all": [round(t, 3) for t in all_torch]}), flush=True)
    print("sequence_bench irradiance done")


def irradiance_horizon(ks, dev):
    """--irradiance-horizon: irradiance()'s workload (n = 2^20 normals on the sphere, RGB, 64 x 256
    cells) under horizon profiles of H = 32 sectors, one shared and one per receiver (sin of the
    elevation uniform in [0, 0.5]).  Two yardsticks of the same session: (a) sequence.irradiance at
    the same n, the ratio the extra multiply per cell and the profile loads cost; (b) what a user
    writes today from the tables read back once -- irradiance()'s chunked torch formulation with
    the visible share v (an n x cells mask per chunk) and the suns' visibility multiplied in.
    Prints the medians, both ratios and the largest difference of the two results."""
    n, chunk, sectors = 1 << 20, 1 << 14, 32
    g = torch.Generator(device=dev).manual_seed(3)
    v = torch.randn((3, n), device=dev, generator=g)
    nrm = (v / v.norm(dim=0, keepdim=True)).contiguous()
    h_per = (0.5 * torch.rand((sectors, n), device=dev, generator=g)).contiguous()
    h_shared = h_per[:, 0].contiguous()
    base = {"type": "sunsky", "sun_direction": [0.3, 0.4, 0.866], "turbidity": 3.0, "albedo": 0.2}
    for k in ks:
        dirs, turb, wts = frames(k)
        seq = ss.SunskySequence(ss.load_dict(dict(base)), dirs, turb, wts)
        seq.prepare_irradiance()
        info = seq.irradiance_info()
        nz, nphi = info["n_z"], info["n_phi"]
        length = nphi // sectors
        z = (np.arange(nz) + 0.5) / nz
        phi = (np.arange(nphi) + 0.5) * (2 * np.pi / nphi)
        st = np.sqrt(1 - z * z)
        D = np.stack([np.outer(st, np.cos(phi)).ravel(), np.outer(st, np.sin(phi)).ravel(), np.repeat(z, nphi)], 1)
        D_t = torch.from_numpy(D.astype(np.float32)).to(dev)                                        # (cells, 3)
        R_t = torch.from_numpy(info["omega"] * seq.irradiance_table("sky").reshape(3, -1)).to(dev)   # (3, cells)
        S_t = torch.from_numpy(np.stack([seq.frame(i)["sun_dir_local"] for i in range(k)])).to(dev)  # (K, 3)
        F_t = torch.from_numpy(wts[None, :] * seq.irradiance_table("sun_flux")).to(dev)              # (3, K)
        sun_sector = torch.from_numpy(seq.irradiance_sun_columns().astype(np.int64) // length).to(dev)   # (K,)
        top = torch.arange(1, nz + 1, device=dev, dtype=torch.float32)
        out_t = torch.empty((3, n), device=dev)
        out = torch.empty((3, n), device=dev)
        out_s = torch.empty((3, n), device=dev)
        out_0 = torch.empty((3, n), device=dev)

        def torch_chunks(h):
            for a in range(0, n, chunk):
                nl = nrm[:, a:a + chunk].t()
                hc = (h[:, a:a + chunk] if h.dim() == 2 else h[:, None].expand(sectors, nl.shape[0])).t()   # (c, H)
                vis = (top[None, :, None] - hc[:, None, :] * nz).clamp_(0, 1)                                # (c, nz, H)
                vis = vis.repeat_interleave(length, dim=2).reshape(nl.shape[0], -1)                          # (c, cells)
                seen = S_t[None, :, 2] >= hc[:, sun_sector]                                                  # (c, K)
                e = (torch.relu(nl @ D_t.t()) * vis) @ R_t.t() + (torch.relu(nl @ S_t.t()) * seen) @ F_t.t()
                out_t[:, a:a + chunk] = e.t()

        t_plain, all_plain = median_ms(lambda: seq.irradiance(nrm, out=out_0))
        t_per, all_per = median_ms(lambda: seq.irradiance(nrm, out=out, horizon=h_per))
        t_shared, all_shared = median_ms(lambda: seq.irradiance(nrm, out=out_s, horizon=h_shared))
        t_torch, all_torch = median_ms(lambda: torch_chunks(h_per))
        diff = float(((out - out_t).abs().max() / out_t.abs().max()).item())
        torch_chunks(h_shared)
        torch.cuda.synchronize()
        diff_s = float(((out_s - out_t).abs().max() / out_t.abs().max()).item())
        print(json.dumps({"K": k, "n": n, "table": [nz, nphi], "sectors": sectors,
                          "irradiance_ms": round(t_plain, 3), "horizon_per_receiver_ms": round(t_per, 3),
                          "horizon_shared_ms": round(t_shared, 3), "torch_masked_chunked_ms": round(t_torch, 3),
                          "per_receiver_over_irradiance": round(t_per / t_plain, 3),
                          "shared_over_irradiance": round(t_shared / t_plain, 3),
                          "torch_over_per_receiver": round(t_torch / t_per, 2),
                          "occluded_share_of_E": round(float((1 - out.sum() / out_0.sum()).item()), 4),
                          "max_diff_vs_torch_of_max": diff, "max_diff_vs_torch_of_max_shared": diff_s,
                          "irradiance_ms_all": [round(t, 3) for t in all_plain],
                          "horizon_per_receiver_ms_all": [round(t, 3) for t in all_per],
                          "horizon_shared_ms_all": [round(t, 3) for t in all_shared],
                          "torch_masked_chunked_ms_all": [round(t, 3) for t in all_torch]}), flush=True)
    print("sequence_bench irradiance-horizon done")


def irradiance_grad(ks, dev):
    """--irradiance-grad: sequence.irradiance_vjp on irradiance()'s workload (n = 2^20 normals on the
    sphere, RGB, 64 x 256 cells) with a standard-normal cotangent: the normal gradient alone, the
    weight gradient alone and both.  Two yardsticks of the same session: (a) sequence.irradiance at
    the same n; (b) what a user writes today -- normals: torch autograd through irradiance()'s
    chunked formulation; weights: a (K P) x cells per-frame table read back from K one-hot
    sequences (timed once, apart), then relu(N_l D^T) @ table^T contracted with the cotangent, in
    chunks.  Prints the medians, the ratios and the largest differences of the results."""
    n, chunk = 1 << 20, 1 << 14
    g = torch.Generator(device=dev).manual_seed(3)
    v = torch.randn((3, n), device=dev, generator=g)
    nrm = (v / v.norm(dim=0, keepdim=True)).contiguous()
    d_out = torch.randn((3, n), device=dev, generator=g)
    base = {"type": "sunsky", "sun_direction": [0.3, 0.4, 0.866], "turbidity": 3.0, "albedo": 0.2}
    for k in ks:
        dirs, turb, wts = frames(k)
        seq = ss.SunskySequence(ss.load_dict(dict(base)), dirs, turb, wts)
        seq.prepare_irradiance()
        t0 = time.perf_counter()
        seq.prepare_irradiance_grad()
        t_prep = (time.perf_counter() - t0) * 1e3
        info = seq.irradiance_info()
        nz, nphi, omega = info["n_z"], info["n_phi"], info["omega"]
        z = (np.arange(nz) + 0.5) / nz
        phi = (np.arange(nphi) + 0.5) * (2 * np.pi / nphi)
        st = np.sqrt(1 - z * z)
        D = np.stack([np.outer(st, np.cos(phi)).ravel(), np.outer(st, np.sin(phi)).ravel(), np.repeat(z, nphi)], 1)
        D_t = torch.from_numpy(D.astype(np.float32)).to(dev)                                        # (cells, 3)
        R_t = torch.from_numpy(omega * seq.irradiance_table("sky").reshape(3, -1)).to(dev)          # (3, cells)
        S_t = torch.from_numpy(np.stack([seq.frame(i)["sun_dir_local"] for i in range(k)])).to(dev)  # (K, 3)
        flux = seq.irradiance_table("sun_flux")                                                      # (3, K)
        F_t = torch.from_numpy(wts[None, :] * flux).to(dev)
        # (b) weights: the per-frame tables from one-hot sequences, once
        t0 = time.perf_counter()
        one = ss.SunskySequence(ss.load_dict(dict(base)), dirs, turb, wts)
        rows = []
        for i in range(k):
            one.update(weights=np.eye(k, dtype=np.float32)[i])
            one.prepare_irradiance()
            rows.append(omega * one.irradiance_table("sky").reshape(3, -1))
        T_t = torch.from_numpy(np.stack(rows).astype(np.float32)).to(dev)                           # (K, 3, cells)
        torch.cuda.synchronize()
        t_tables = (time.perf_counter() - t0) * 1e3
        Fk_t = torch.from_numpy(np.ascontiguousarray(flux.T)).to(dev)                                # (K, 3)
        out = torch.empty((3, n), device=dev)
        gn, gw = torch.empty((3, n), device=dev), torch.zeros(k, device=dev)
        gn_t, gw_t = torch.empty((3, n), device=dev), torch.zeros(k, device=dev)

        def torch_normals():
            for a in range(0, n, chunk):
                nl = nrm[:, a:a + chunk].t().detach().requires_grad_(True)
                e = torch.relu(nl @ D_t.t()) @ R_t.t() + torch.relu(nl @ S_t.t()) @ F_t.t()
                (e * d_out[:, a:a + chunk].t()).sum().backward()
                gn_t[:, a:a + chunk] = nl.grad.t()

        def torch_weights():
            gw_t.zero_()
            for a in range(0, n, chunk):
                nl, dd = nrm[:, a:a + chunk].t(), d_out[:, a:a + chunk].t()                          # (c, 3) each
                ek = (torch.relu(nl @ D_t.t()) @ T_t.reshape(3 * k, -1).t()).reshape(-1, k, 3)       # (c, K, 3)
                ek = ek + torch.relu(nl @ S_t.t())[:, :, None] * Fk_t[None]
                gw_t.add_((ek * dd[:, None, :]).sum((0, 2)))

        def vjp_weights():
            gw.zero_()
            seq.irradiance_vjp(nrm, d_out, grad={"normals": None, "weights": gw})

        t_fwd, all_fwd = median_ms(lambda: seq.irradiance(nrm, out=out))
        t_n, all_n = median_ms(lambda: seq.irradiance_vjp(nrm, d_out, grad={"normals": gn, "weights": None}))
        t_w, all_w = median_ms(vjp_weights)
        t_both, all_both = median_ms(lambda: seq.irradiance_vjp(nrm, d_out, grad={"normals": gn, "weights": gw}))
        t_tn, all_tn = median_ms(torch_normals)
        t_tw, all_tw = median_ms(torch_weights)
        vjp_weights()
        torch.cuda.synchronize()
        pairs = n * (nz * nphi + k)
        print(json.dumps({"K": k, "n": n, "table": [nz, nphi], "prepare_irradiance_grad_ms": round(t_prep, 3),
                          "irradiance_ms": round(t_fwd, 3), "vjp_normals_ms": round(t_n, 3),
                          "vjp_weights_ms": round(t_w, 3), "vjp_both_ms": round(t_both, 3),
                          "normals_over_forward": round(t_n / t_fwd, 2), "weights_over_forward": round(t_w / t_fwd, 2),
                          "both_over_forward": round(t_both / t_fwd, 2),
                          "torch_normals_ms": round(t_tn, 3), "torch_weights_ms": round(t_tw, 3),
                          "torch_weights_tables_once_ms": round(t_tables, 1),
                          "torch_over_vjp_normals": round(t_tn / t_n, 2), "torch_over_vjp_weights": round(t_tw / t_w, 2),
                          "normals_pairs_per_s": round(pairs / (t_n * 1e-3), 0),
                          "weights_pairs_per_s": round(pairs / (t_w * 1e-3), 0),
                          "max_diff_normals_of_max": float(((gn - gn_t).abs().max() / gn_t.abs().max()).item()),
                          "max_diff_weights_of_max": float(((gw - gw_t).abs().max() / gw_t.abs().max()).item()),
                          "irradiance_ms_all": [round(t, 3) for t in all_fwd],
                          "vjp_normals_ms_all": [round(t, 3) for t in all_n],
                          "vjp_weights_ms_all": [round(t, 3) for t in all_w],
                          "vjp_both_ms_all": [round(t, 3) for t in all_both],
                          "torch_normals_ms_all": [round(t, 3) for t in all_tn],
                          "torch_weights_ms_all": [round(t, 3) for t in all_tw]}), flush=True)
    print("sequence_bench irradiance-grad done")


def irradiance_horizon_grad(ks, dev):
    """--irradiance-horizon-grad: sequence.irradiance_vjp(horizon=...) on irradiance_horizon()'s workload
    (n = 2^20 normals on the sphere, RGB, 64 x 256 cells, H = 32 sectors, sin of the elevation
    uniform in [0, 0.5]) with a standard-normal cotangent: each gradient alone and all three, for a
    shared and for per-receiver profiles.  Yardsticks of the same session, all existing code:
    (a) irradiance_vjp (open) at the same n; (b) irradiance(horizon=); (c) what a user writes today
    -- torch autograd through irradiance_horizon()'s masked chunked formulation, differentiated in
    the normals and the profile, and for the weights irradiance_grad()'s per-frame table (here from
    irradiance_frame_table) contracted with the masked cosines.  Prints the medians, the ratios and
    the largest differences to (c).  The profile's gradient jumps where h n_z crosses an integer
    (another row becomes the partly covered one), and torch forms i + 1 - h n_z with two roundings
    where the kernel has one fma: the few entries within 1e-5 of such a crossing are counted and
    left out of that difference."""
    n, chunk, sectors = 1 << 20, 1 << 14, 32
    g = torch.Generator(device=dev).manual_seed(3)
    v = torch.randn((3, n), device=dev, generator=g)
    nrm = (v / v.norm(dim=0, keepdim=True)).contiguous()
    h_per = (0.5 * torch.rand((sectors, n), device=dev, generator=g)).contiguous()
    h_shared = h_per[:, 0].contiguous()
    d_out = torch.randn((3, n), device=dev, generator=g)
    base = {"type": "sunsky", "sun_direction": [0.3, 0.4, 0.866], "turbidity": 3.0, "albedo": 0.2}
    for k in ks:
        dirs, turb, wts = frames(k)
        seq = ss.SunskySequence(ss.load_dict(dict(base)), dirs, turb, wts)
        seq.prepare_irradiance()
        seq.prepare_irradiance_grad()
        info = seq.irradiance_info()
        nz, nphi, omega = info["n_z"], info["n_phi"], info["omega"]
        length = nphi // sectors
        z = (np.arange(nz) + 0.5) / nz
        phi = (np.arange(nphi) + 0.5) * (2 * np.pi / nphi)
        st = np.sqrt(1 - z * z)
        D = np.stack([np.outer(st, np.cos(phi)).ravel(), np.outer(st, np.sin(phi)).ravel(), np.repeat(z, nphi)], 1)
        D_t = torch.from_numpy(D.astype(np.float32)).to(dev)                                        # (cells, 3)
        R_t = torch.from_numpy(omega * seq.irradiance_table("sky").reshape(3, -1)).to(dev)          # (3, cells)
        S_t = torch.from_numpy(np.stack([seq.frame(i)["sun_dir_local"] for i in range(k)])).to(dev)  # (K, 3)
        flux = seq.irradiance_table("sun_flux")                                                      # (3, K)
        F_t = torch.from_numpy(wts[None, :] * flux).to(dev)
        Fk_t = torch.from_numpy(np.ascontiguousarray(flux.T)).to(dev)                                # (K, 3)
        T_t = torch.from_numpy(np.stack([omega * seq.irradiance_frame_table(i).reshape(3, -1) for i in range(k)])
                               .astype(np.float32)).to(dev)                                         # (K, 3, cells)
        sun_sector = torch.from_numpy(seq.irradiance_sun_columns().astype(np.int64) // length).to(dev)
        top = torch.arange(1, nz + 1, device=dev, dtype=torch.float32)
        out = torch.empty((3, n), device=dev)
        gn, gw, gh = torch.empty((3, n), device=dev), torch.zeros(k, device=dev), torch.empty((sectors, n), device=dev)
        gn_t, gw_t, gh_t = torch.empty((3, n), device=dev), torch.zeros(k, device=dev), torch.empty((sectors, n), device=dev)

        def masks(nl, hc):
            vis = (top[None, :, None] - hc[:, None, :] * nz).clamp(0, 1)                           # (c, nz, H)
            vis = vis.repeat_interleave(length, dim=2).reshape(nl.shape[0], -1)                      # (c, cells)
            return vis, S_t[None, :, 2] >= hc[:, sun_sector]                                         # (c, K)

        def torch_normals_and_profile():
            for a in range(0, n, chunk):
                nl = nrm[:, a:a + chunk].t().detach().requires_grad_(True)
                hc = h_per[:, a:a + chunk].t().detach().requires_grad_(True)
                vis, seen = masks(nl, hc)
                e = (torch.relu(nl @ D_t.t()) * vis) @ R_t.t() + (torch.relu(nl @ S_t.t()) * seen) @ F_t.t()
                (e * d_out[:, a:a + chunk].t()).sum().backward()
                gn_t[:, a:a + chunk] = nl.grad.t()
                gh_t[:, a:a + chunk] = hc.grad.t()

        def torch_weights():
            gw_t.zero_()
            with torch.no_grad():
                for a in range(0, n, chunk):
                    nl, dd = nrm[:, a:a + chunk].t(), d_out[:, a:a + chunk].t()
                    vis, seen = masks(nl, h_per[:, a:a + chunk].t())
                    ek = ((torch.relu(nl @ D_t.t()) * vis) @ T_t.reshape(3 * k, -1).t()).reshape(-1, k, 3)
                    ek = ek + (torch.relu(nl @ S_t.t()) * seen)[:, :, None] * Fk_t[None]
                    gw_t.add_((ek * dd[:, None, :]).sum((0, 2)))

        def vjp(h, normals=False, weights=False, horizon=False):
            def step():
                if weights:
                    gw.zero_()
                buf = None if not horizon else gh if h.dim() == 2 else torch.empty(sectors, device=dev)
                seq.irradiance_vjp(nrm, d_out, grad={"normals": gn if normals else None, "weights": gw if weights else None,
                                                     "horizon": buf}, horizon=h)
            return step

        def open_weights():
            gw.zero_()
            seq.irradiance_vjp(nrm, d_out, grad={"normals": None, "weights": gw})

        line = {"K": k, "n": n, "table": [nz, nphi], "sectors": sectors}
        alls = {}

        def timed(name, step):
            t, ts = median_ms(step)
            line[name + "_ms"] = round(t, 3)
            alls[name + "_ms_all"] = [round(x, 3) for x in ts]
            return t

        t_on = timed("open_vjp_normals", lambda: seq.irradiance_vjp(nrm, d_out, grad={"normals": gn, "weights": None}))
        t_ow = timed("open_vjp_weights", open_weights)
        t_ob = timed("open_vjp_both", lambda: seq.irradiance_vjp(nrm, d_out, grad={"normals": gn, "weights": gw}))
        t_f = timed("irradiance_horizon_per_receiver", lambda: seq.irradiance(nrm, out=out, horizon=h_per))
        timed("irradiance_horizon_shared", lambda: seq.irradiance(nrm, out=out, horizon=h_shared))
        t = {}
        for kind, h in (("per_receiver", h_per), ("shared", h_shared)):
            t[kind, "n"] = timed(f"{kind}_normals", vjp(h, normals=True))
            t[kind, "w"] = timed(f"{kind}_weights", vjp(h, weights=True))
            t[kind, "h"] = timed(f"{kind}_horizon", vjp(h, horizon=True))
            t[kind, "nh"] = timed(f"{kind}_normals_and_horizon", vjp(h, normals=True, horizon=True))
            t[kind, "all"] = timed(f"{kind}_all_three", vjp(h, normals=True, weights=True, horizon=True))
            line[f"{kind}_normals_over_open"] = round(t[kind, "n"] / t_on, 3)
            line[f"{kind}_weights_over_open"] = round(t[kind, "w"] / t_ow, 3)
            line[f"{kind}_normals_and_horizon_over_normals"] = round(t[kind, "nh"] / t[kind, "n"], 3)
            line[f"{kind}_all_three_over_open_both"] = round(t[kind, "all"] / t_ob, 3)
            line[f"{kind}_all_three_over_forward"] = round(t[kind, "all"] / t_f, 3)
        t_tn = timed("torch_normals_and_profile", torch_normals_and_profile)
        t_tw = timed("torch_weights", torch_weights)
        vjp(h_per, normals=True, weights=True, horizon=True)()
        torch.cuda.synchronize()
        line.update({"torch_over_normals_and_horizon": round(t_tn / t["per_receiver", "nh"], 2),
                     "torch_over_weights": round(t_tw / t["per_receiver", "w"], 2),
                     "torch_over_all_three": round((t_tn + t_tw) / t["per_receiver", "all"], 2),
                     "max_diff_normals_of_max": float(((gn - gn_t).abs().max() / gn_t.abs().max()).item()),
                     "max_diff_weights_of_max": float(((gw - gw_t).abs().max() / gw_t.abs().max()).item())})
        x = h_per * nz
        at_jump = (x - x.round()).abs() < 1e-5
        dh = (gh - gh_t).abs() / gh_t.abs().max()
        line.update({"max_diff_horizon_of_max": float(dh[~at_jump].max().item()),
                     "horizon_entries_at_a_row_crossing": int(at_jump.sum().item()),
                     "max_diff_horizon_of_max_at_a_row_crossing": float(dh[at_jump].max().item()) if bool(at_jump.any()) else 0.0})
        line.update(alls)
        print(json.dumps(line), flush=True)
    print("sequence_bench irradiance-horizon-grad done")


def irradiance_series(ks, dev):
    """--irradiance-series: every frame's own irradiance on 2^20 receivers (RGB, normals uniform on
    the sphere, 64 x 256 cells) in one call per frame sub-range, open and under per-receiver
    horizons of 32 sectors, against two yardsticks of the same session: (a) irradiance() of the
    weighted sequence once, and (b) what a user writes without the series, K one-frame sequences
    prepared beforehand (their preparation not counted), each irradiance() into its slice.

    The output of K frames is K x 3 x n floats (4.6 GB at K = 365), so both sides write sub-ranges
    of at most 64 frames (a multiple of the group size, so no group is walked twice) into one
    reused 64 x 3 x n buffer; a time is the sum over the sub-ranges.  The largest difference to
    (b), which must be 0, is taken sub-range by sub-range in an untimed pass.

    The derived issue floor: per record, receiver pair and group of 8 frames 5 + 24 wave
    instructions of 4 cycles on 1024 SIMDs, at the GFX clock polled while the series runs."""
    n, nz, nphi, sectors, span = 1 << 20, 64, 256, 32, 64
    g = torch.Generator(device=dev).manual_seed(5)
    v = torch.randn((3, n), device=dev, generator=g)
    nrm = (v / v.norm(dim=0, keepdim=True)).contiguous()
    hz = (torch.rand((sectors, n), device=dev, generator=g) * 1.4 - 0.2).contiguous()
    base = {"type": "sunsky", "sun_direction": [0.3, 0.4, 0.866], "turbidity": 3.0, "albedo": 0.2}
    for k in ks:
        dirs, turb, wts = frames(k)
        parent = ss.load_dict(dict(base))
        seq = ss.SunskySequence(parent, dirs, turb, wts)
        seq.prepare_irradiance(nz, nphi)
        t0 = time.perf_counter()
        seq.prepare_irradiance_series()
        t_prep = (time.perf_counter() - t0) * 1e3
        ones = []
        for i in range(k):
            one = ss.SunskySequence(parent, dirs[i:i + 1], turb[i:i + 1], [1.0])
            one.prepare_irradiance(nz, nphi)
            ones.append(one)
        group = ss._capi.seq_irr_series_group(3)
        assert span % group == 0
        ranges = [(f, min(span, k - f)) for f in range(0, k, span)]
        buf, buf_b = torch.empty((min(span, k), 3, n), device=dev), torch.empty((min(span, k), 3, n), device=dev)
        out = torch.empty((3, n), device=dev)

        def series(horizon=None):
            for f, c in ranges:
                seq.irradiance_series(nrm, frames=(f, c), out=buf[:c], horizon=horizon)

        def loop(horizon=None, f0=0, count=k):
            for i in range(f0, f0 + count):
                ones[i].irradiance(nrm, out=buf_b[(i - f0) % span], horizon=horizon)

        def clock_during(step):
            """Median GFX clock in MHz polled on the host while step's launches run (None: no reading)."""
            done = torch.cuda.Event()
            samples = []
            try:
                step()
                done.record()
                while not done.query():
                    samples.append(torch.cuda.clock_rate())
            except Exception:
                samples = []
            torch.cuda.synchronize()
            return statistics.median(samples) if samples else None

        line = {"K": k, "n": n, "table": [nz, nphi], "group": group, "sub_ranges": len(ranges),
                "prepare_irradiance_series_ms": round(t_prep, 3)}
        t_once, all_once = median_ms(lambda: seq.irradiance(nrm, out=out))
        line["irradiance_once_ms"] = round(t_once, 3)
        for name, horizon in (("open", None), ("horizon", hz)):
            t_s, all_s = median_ms(lambda: series(horizon))
            t_b, all_b = median_ms(lambda: loop(horizon))
            mhz = clock_during(lambda: series(horizon))
            worst = 0.0
            for f, c in ranges:   # untimed: the two sides of every sub-range, bit for bit
                seq.irradiance_series(nrm, frames=(f, c), out=buf[:c], horizon=horizon)
                loop(horizon, f, c)
                worst = max(worst, float((buf[:c] - buf_b[:c]).abs().max().item()))
            work = n * nz * nphi * k
            line[name] = {"series_ms": round(t_s, 3), "one_frame_loop_ms": round(t_b, 3), "loop_over_series": round(t_b / t_s, 3),
                          "receiver_cell_frames_per_s": round(work / (t_s * 1e-3), 0),
                          "max_abs_diff_to_loop": worst,
                          "series_ms_all": [round(t, 3) for t in all_s], "one_frame_loop_ms_all": [round(t, 3) for t in all_b]}
            if mhz:
                groups = -(-k // group)
                floor_ms = (n / 128) * nz * nphi * groups * 29 * 4 / (1024 * mhz * 1e6) * 1e3
                line[name].update({"gfx_clock_mhz": mhz, "issue_floor_ms": round(floor_ms, 3),
                                   "share_of_issue_floor": round(floor_ms / t_s, 3)})
        line["irradiance_once_ms_all"] = [round(t, 3) for t in all_once]
        print(json.dumps(line), flush=True)
        del ones, buf, buf_b
    print("sequence_bench irradiance-series done")


def main():
    flags = ("--sampling", "--grad", "--no-loop", "--irradiance", "--irradiance-grad", "--irradiance-horizon",
             "--irradiance-series", "--irradiance-horizon-grad")
    args = [a for a in sys.argv[1:] if a not in flags]
    ks = [int(a) for a in args] or [24, 365]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if "--sampling" in sys.argv[1:]:
        return sampling(ks, dev)
    if "--irradiance-horizon-grad" in sys.argv[1:]:
        return irradiance_horizon_grad(ks, dev)
    if "--irradiance-series" in sys.argv[1:]:
        return irradiance_series(ks, dev)
    if "--irradiance" in sys.argv[1:]:
        return irradiance(ks, dev)
    if "--irradiance-grad" in sys.argv[1:]:
        return irradiance_grad(ks, dev)
    if "--irradiance-horizon" in sys.argv[1:]:
        return irradiance_horizon(ks, dev)
    if "--grad" in sys.argv[1:]:
        return grad(ks, dev, "--no-loop" not in sys.argv[1:])
    g = torch.Generator(device=dev).manual_seed(3)
    v = torch.randn((3, N), device=dev, generator=g)
    v[2] = v[2].abs()
    wi = -(v / v.norm(dim=0, keepdim=True)).contiguous()
    si = ss.SurfaceInteraction3f(wi=wi)
    base = {"type": "sunsky", "sun_direction": [0.3, 0.4, 0.866], "turbidity": 3.0, "albedo": 0.2}
    for k in ks:
        dirs, turb, wts = frames(k)
        em = ss.load_dict(dict(base))
        params = em.traverse()
        out_loop = torch.empty((3, N), device=dev)

        def baseline():
            out_loop.zero_()
            for i in range(k):
                params["sun_direction"] = dirs[i]
                params["turbidity"] = float(turb[i])
                params.update()
                out_loop.add_(em.eval(si), alpha=float(wts[i]))

        seq = ss.SunskySequence(ss.load_dict(dict(base)), dirs, turb, wts)
        out_seq = torch.empty((3, N), device=dev)
        t_seq, all_seq = median_ms(lambda: seq.eval(wi, out=out_seq))
        t_base, all_base = median_ms(baseline)
        # Agreement of the two paths.  set_param stages a sun direction as given while a sequence
        # normalises it like the constructor: an ulp on the sun vector moves the fp32 disc test
        # dot >= cos_cutoff by ~0.5 % of the disc's solid angle (1 - cos_cutoff = 1.1e-5), so a few
        # disc-edge lanes per run sit on different sides; every other lane agrees to rounding.
        rel = (out_seq - out_loop).abs() / out_loop.abs().clamp_min(1e-6 * out_loop.abs().max().item())
        lanes_off = int((rel > 1e-4).any(dim=0).sum().item())
        rel_q = float(rel.flatten()[:: 7].quantile(0.999).item())
        print(json.dumps({"K": k, "n": N, "baseline_ms": round(t_base, 3), "sequence_ms": round(t_seq, 3),
                          "speedup": round(t_base / t_seq, 2),
                          "frame_evals_per_s": round(N * k / (t_seq * 1e-3), 0),
                          "baseline_evals_per_s": round(N * k / (t_base * 1e-3), 0),
                          "lanes_over_1e-4_vs_loop": lanes_off, "rel_diff_q999": rel_q,
                          "sequence_ms_all": [round(t, 3) for t in all_seq],
                          "baseline_ms_all": [round(t, 3) for t in all_base]}), flush=True)
    print("sequence_bench done")


if __name__ == "__main__":
    main()
