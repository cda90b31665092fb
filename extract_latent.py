"""Latent extraction: images -> VAE moments on disk, the input of train.py / train_wds.py (counterpart of the reference's
extract_latent.py).

    python extract_latent.py --data_dir ../datasets --split train --ckpt assets/vae/autoencoder_kl.pth \\
        --resolution 256 --batch_size 64 --xflip --outdir ../data/imagenet256-latent [--format wds|lmdb]

Input: an ImageFolder tree <data_dir>/<split>/<class>/<image> (labels = sorted class-directory index, class-major order
as torchvision's ImageFolder; maskdit_amd.images).  Every image is decoded to RGB and center-cropped (ADM) on a pool of
host threads, one batch ahead of the GPU, and goes to the device as uint8; FrozenAutoencoderKL.encode_moments applies
ToTensor + Normalize(0.5, 0.5) there.  Output under <outdir>/<data_name>_<resolution>_latent_<format>/<split>:
  lmdb: the reference's records -- `z-{i}` raw float32 moments [8, R/8, R/8], `y-{i}` label text, `length`
        (maskdit_amd.data.LmdbLatents reads it; needs the `lmdb` module)
  wds : tar shards of --shard_size samples (`<key>.latent` pickle + `<key>.cls`, key = global index;
        maskdit_amd.data.WdsTarLatents / train_wds.py read them)
--xflip stores the mirrored images' moments after the N originals (indices N .. 2N-1), as the reference does.
--rank / --world (wds only): this process encodes the contiguous slice rank of world (and its mirrored copies) into
shards of its own, so several GPUs split one dataset.  --ckpt none: seeded synthetic weights (--seed).
--vae_precision bf16x3: the encoder at the reference's fp32 accuracy (default bf16: bf16 operands)."""
import argparse
import concurrent.futures as cf
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from maskdit_amd import autoencoder as AE  # noqa: E402
from maskdit_amd.data import write_wds_shard  # noqa: E402
from maskdit_amd.images import image_folder_samples, load_rgb_crop  # noqa: E402


class WdsSink:
    """Consecutive samples from global index `start` on, flushed into shards of `size` samples."""

    def __init__(self, outdir, tag, start, size):
        self.outdir, self.tag, self.start, self.size = outdir, tag, start, size
        self.z, self.y, self.n = [], [], 0

    def put(self, z, y):
        self.z.extend(z)
        self.y.extend(y)
        while len(self.z) >= self.size:
            self._flush(self.size)

    def _flush(self, k):
        path = os.path.join(self.outdir, f'{self.tag}-{self.start + self.n:09d}.tar')
        write_wds_shard(path, self.z[:k], self.y[:k], start_index=self.start + self.n)
        self.z, self.y, self.n = self.z[k:], self.y[k:], self.n + k

    def close(self):
        if self.z:
            self._flush(len(self.z))


class LmdbSink:
    def __init__(self, env, start):
        self.env, self.i = env, start

    def put(self, z, y):
        with self.env.begin(write=True) as txn:
            for m, lb in zip(z, y):
                txn.put(f'z-{self.i}'.encode('utf-8'), np.ascontiguousarray(m, dtype=np.float32).tobytes())
                txn.put(f'y-{self.i}'.encode('utf-8'), str(int(lb)).encode('utf-8'))
                self.i += 1

    def close(self):
        pass


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--data_name', default='imagenet', type=str)
    ap.add_argument('--data_dir', default='../datasets', type=str)
    ap.add_argument('--ckpt', default='assets/vae/autoencoder_kl.pth', type=str, help="checkpoint path, or 'none'")
    ap.add_argument('--seed', default=0, type=int, help='synthetic weights of --ckpt none')
    ap.add_argument('--resolution', default=512, type=int, choices=AE.ENC_SIDES)
    ap.add_argument('--batch_size', default=128, type=int)
    ap.add_argument('--split', default='train', type=str, choices=['train', 'val'])
    ap.add_argument('--xflip', action='store_true')
    ap.add_argument('--outdir', type=str, default='../data/imagenet512-latent', help='output directory')
    ap.add_argument('--format', default='wds', choices=['wds', 'lmdb'])
    ap.add_argument('--shard_size', default=1000, type=int, help='samples per tar shard (wds)')
    ap.add_argument('--rank', default=0, type=int)
    ap.add_argument('--world', default=1, type=int)
    ap.add_argument('--workers', default=16, type=int, help='host decode threads (at most 16)')
    ap.add_argument('--device', default='cuda', type=str)
    ap.add_argument('--vae_precision', default='bf16', choices=list(AE.PRECISIONS),
                    help="encoder arithmetic: 'bf16x3' = the reference's fp32 accuracy, 'bf16' = bf16 operands (default)")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.format == 'lmdb' and args.world != 1:
        ap.error('--rank / --world split the dataset into WebDataset shards: use --format wds')
    if not 0 <= args.rank < args.world:
        ap.error('need 0 <= rank < world')

    samples, classes = image_folder_samples(os.path.join(args.data_dir, args.split))
    N = len(samples)
    lo, hi = N * args.rank // args.world, N * (args.rank + 1) // args.world
    print(f'data size: {N} images in {len(classes)} classes; rank {args.rank}/{args.world} encodes [{lo}, {hi})')

    if args.ckpt.lower() == 'none':
        vae = AE.get_model(None, encoder=True, precision=args.vae_precision)
        vae.load_state_dict(AE.synthetic_state_dict(args.seed))
        print(f'synthetic VAE weights (seed {args.seed})')
    else:
        vae = AE.get_model(args.ckpt, encoder=True, precision=args.vae_precision)
        print(f'load vae weights from {args.ckpt}')
    dev = torch.device(args.device)
    vae = vae.to(dev)

    target = os.path.join(args.outdir, f'{args.data_name}_{args.resolution}_latent_{args.format}', args.split)
    os.makedirs(target, exist_ok=True)
    env = None
    if args.format == 'lmdb':
        try:
            import lmdb
        except ImportError:
            sys.exit('extract_latent.py: --format lmdb needs the `lmdb` Python module, which is not installed '
                     '(use --format wds, or install lmdb)')
        env = lmdb.open(target, map_size=pow(2, 40), readahead=False)
        sinks = [LmdbSink(env, lo)] + ([LmdbSink(env, N + lo)] if args.xflip else [])
    else:
        tag = f'shard-r{args.rank:03d}'
        sinks = [WdsSink(target, tag, lo, args.shard_size)]
        if args.xflip:
            sinks.append(WdsSink(target, tag + '-xflip', N + lo, args.shard_size))

    R, bs = args.resolution, args.batch_size
    pool = cf.ThreadPoolExecutor(max_workers=max(1, min(16, args.workers)))
    starts = list(range(lo, hi, bs))

    def submit(s):
        return [pool.submit(load_rgb_crop, samples[i][0], R) for i in range(s, min(s + bs, hi))]

    pending = submit(starts[0]) if starts else []
    t0, done = time.time(), 0
    for k, s in enumerate(starts):
        futs = pending
        pending = submit(starts[k + 1]) if k + 1 < len(starts) else []  # decode the next batch while this one encodes
        batch = np.stack([f.result() for f in futs])
        labels = [samples[i][1] for i in range(s, s + len(futs))]
        x = torch.from_numpy(batch).pin_memory().to(dev, non_blocking=True)
        moms = [vae.encode_moments(x)]
        if args.xflip:
            moms.append(vae.encode_moments(x, flip=True))  # img.flip(dims=[-1]) (reference extract_latent.py:91)
        for sink, m in zip(sinks, moms):
            sink.put(list(m.cpu().numpy()), labels)
        done += len(futs)
        if k % 20 == 0 or done == hi - lo:
            dt = time.time() - t0
            print(f'encoded {done}/{hi - lo} images, {done / max(dt, 1e-9):.1f} img/s')
    pool.shutdown()
    for sink in sinks:
        sink.close()
    total = (hi - lo) * (2 if args.xflip else 1)
    if env is not None:
        with env.begin(write=True) as txn:
            txn.put('length'.encode('utf-8'), str(total).encode('utf-8'))
        env.close()
    dt = time.time() - t0
    print(f'[finished] saved {total} latents to {target} in {dt:.1f} s ({(hi - lo) / max(dt, 1e-9):.1f} images/s)')
    return 0


if __name__ == '__main__':
    sys.exit(main())
