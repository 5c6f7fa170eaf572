"""What does the device-resident dataset (device_data.py, csrc/input_pipeline.hip) cost and save?  Writes a synthetic Labelme dataset of
native-size PNG tiles to a temporary directory and reports, on one GPU, as medians over interleaved rounds with the rounds' min..max:
(a) the cache build (decode + rasterise on the host, resample on the device) against CoastalDataset with 0 and 16 workers, images/s;
(b) runet_batch_assemble at 16 x size^2 with and without augmentation, and the two resampling passes: device-event time, achieved GB/s from
    the bytes the algorithm has to move; (c) the PIL augmentation chain per image on one core; (d) a RobustUNet training epoch fed by
    DeviceLoader with and without Augment against the step on resident data and against 16 workers + pinned memory + DevicePrefetcher.
The device-event times of (b) are per call of the Python wrapper: for kernels shorter than the host's enqueue time they measure the enqueue.
`--kernels` runs only the kernels of (b) on a random cache, 20 calls each, for a kernel trace:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/bench_device_input.py --kernels [native=1024] [size=512]
usage: python tools/bench_device_input.py [n_images=64] [native=1024] [size=512] [rounds=5]"""
import importlib
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image, ImageEnhance
from torch.utils.data import DataLoader

pkg = importlib.import_module("eusipco-2026-robust-unet_amd")
data = importlib.import_module("eusipco-2026-robust-unet_amd.data")
dd = importlib.import_module("eusipco-2026-robust-unet_amd.device_data")
BATCH = 16


def make_dataset(root, n, native):
    os.makedirs(os.path.join(root, "images")); os.makedirs(os.path.join(root, "labels"))
    rng = np.random.default_rng(0)
    for i in range(n):
        Image.fromarray(rng.integers(0, 255, (native, native, 3), dtype=np.uint8)).save(os.path.join(root, "images", f"t{i:04d}.png"), compress_level=1)
        with open(os.path.join(root, "labels", f"t{i:04d}.json"), "w") as f:
            json.dump({"shapes": data.synthetic_shapes(native, i), "imageHeight": native, "imageWidth": native}, f)


def show(name, values, unit, extra=""):
    print(f"{name}: median {statistics.median(values):.4g} {unit} (min {min(values):.4g}, max {max(values):.4g}, {len(values)} rounds){extra}", flush=True)


def device_ms(fn, reps):
    """milliseconds per call from device events around `reps` calls"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def pil_chain(img, p, k):
    if p["flip"][k]:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    img = img.rotate(float(p["angle"][k]), Image.NEAREST, expand=False, fillcolor=0)
    for j in range(3):
        which = (int(p["order"][k]) >> (2 * j)) & 3
        img = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)[which](img).enhance(float(p["factors"][k][which]))
    return img


def kernel_jobs(images, masks, native, size, dev):
    """{name: (call, least bytes moved)} of the four kernel measurements on a cache [M, size, size, 3]"""
    p = dd.Augment().draw(BATCH, 1, 0)
    index = torch.arange(BATCH, dtype=torch.int32, device=dev) % images.shape[0]
    geom = torch.from_numpy(dd.geometry_words(size, p["flip"], p["angle"], p["order"])).to(dev)
    factors = torch.from_numpy(p["factors"]).to(dev)
    src = torch.randint(0, 256, (native, native, 3), dtype=torch.uint8, device=dev)
    mid = dd.resize_pil_device(src, (size, native), "lanczos")
    npix = BATCH * size * size
    return {
        "assemble, no augmentation": (lambda: dd.assemble_batch(images, masks, index), npix * (4 + 16)),
        "gray sums + assemble, augmentation": (lambda: dd.assemble_batch(images, masks, index, geom=geom, factors=factors), npix * (3 + 4 + 16)),
        "resample rows (horizontal pass)": (lambda: dd.resize_pil_device(src, (size, native), "lanczos"), native * (native + size) * 3),
        "resample cols (vertical pass)": (lambda: dd.resize_pil_device(mid, (size, size), "lanczos"), size * (native + size) * 3),
    }


def kernels_only(native, size):
    dev = torch.device("cuda:0")
    images = torch.randint(0, 256, (BATCH, size, size, 3), dtype=torch.uint8, device=dev)
    masks = torch.randint(0, 2, (BATCH, size, size), dtype=torch.uint8, device=dev)
    for name, (fn, nbytes) in kernel_jobs(images, masks, native, size, dev).items():
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        print(f"{name}: 20 calls, {nbytes / 1e6:.1f} MB moved at least per call", flush=True)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_device_input.py measures on a GPU; none is available")
    if len(sys.argv) > 1 and sys.argv[1] == "--kernels":
        return kernels_only(int(sys.argv[2]) if len(sys.argv) > 2 else 1024, int(sys.argv[3]) if len(sys.argv) > 3 else 512)
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    native = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    size = int(sys.argv[3]) if len(sys.argv) > 3 else 512
    rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    dev = torch.device("cuda:0")
    torch.set_num_threads(1)
    print(f"{n} images {native}^2 -> {size}^2, batch {BATCH}, {rounds} interleaved rounds, device {torch.cuda.get_device_name(0)}", flush=True)
    with tempfile.TemporaryDirectory() as root:
        make_dataset(root, n, native)
        idir, ldir = os.path.join(root, "images"), os.path.join(root, "labels")
        names = sorted(os.listdir(idir))
        ipaths = [os.path.join(idir, f) for f in names]
        lpaths = [os.path.join(ldir, os.path.splitext(f)[0] + ".json") for f in names]
        tf = data.Compose([data.Resize((size, size)), data.ToTensor(), data.Normalize(data.IMAGENET_MEAN, data.IMAGENET_STD)])
        host = data.CoastalDataset(ipaths, lpaths, transform=tf, image_size=(size, size))
        kw = dict(batch_size=BATCH, shuffle=True, pin_memory=True)
        host0 = DataLoader(host, num_workers=0, **kw)
        host16 = DataLoader(host, num_workers=16, persistent_workers=True, **kw)
        for _ in host16:                                     # worker start-up
            pass
        ds = dd.DeviceCoastalDataset(ipaths, lpaths, image_size=(size, size), device=dev)      # warm-up build; kept for (b) and (d)
        torch.cuda.synchronize()

        # ---- (a) cache build against the host dataset, one pass over the files each, interleaved
        res = {"build": [], "host0": [], "host16": []}
        for _ in range(rounds):
            t0 = time.perf_counter()
            dd.DeviceCoastalDataset(ipaths, lpaths, image_size=(size, size), device=dev)
            torch.cuda.synchronize()
            res["build"].append(n / (time.perf_counter() - t0))
            for key, loader in (("host0", host0), ("host16", host16)):
                t0 = time.perf_counter()
                for _b in loader:
                    pass
                res[key].append(n / (time.perf_counter() - t0))
        show("cache build (host decode + rasterise, device resample), once per dataset", res["build"], "img/s")
        show("CoastalDataset, 0 workers, every epoch", res["host0"], "img/s")
        show("CoastalDataset, 16 workers, every epoch", res["host16"], "img/s")

        # ---- (b) kernels
        aug = dd.Augment()
        p = aug.draw(BATCH, 1, 0)
        jobs = kernel_jobs(ds.images, ds.masks, native, size, dev)
        times = {k: [] for k in jobs}
        for k, (fn, _) in jobs.items():
            device_ms(fn, 10)
        for _ in range(rounds):
            for k, (fn, _) in jobs.items():
                times[k].append(device_ms(fn, 50))
        for k, (_, nbytes) in jobs.items():
            med = statistics.median(times[k])
            show(f"{k} [{BATCH} x {size}^2]" if "assemble" in k else f"{k} [{native}^2 -> {size}]", times[k], "ms",
                 f"; {nbytes / 1e6:.1f} MB moved at least -> {nbytes / med / 1e6:.0f} GB/s (per wrapper call: the enqueue time where the kernel is shorter)")

        # ---- (c) the PIL chain on one core
        tiles = [Image.fromarray(ds.images[i % n].cpu().numpy()) for i in range(BATCH)]
        host_ms = []
        for _ in range(rounds):
            t0 = time.perf_counter()
            for k, im in enumerate(tiles):
                pil_chain(im, p, k)
            host_ms.append((time.perf_counter() - t0) * 1e3 / BATCH)
        show(f"PIL flip + rotate + three ImageEnhance passes at {size}^2, one core", host_ms, "ms/img",
             f" -> {1e3 / statistics.median(host_ms):.0f} img/s per core")

        # ---- (d) a training epoch
        model = pkg.RobustUNet(3, 1, 64).to(dev).train()
        step = pkg.TrainStep(model)
        x, y = pkg.synthetic_batch(BATCH, size)
        x, y = x.to(dev), y.to(dev)
        plain = dd.DeviceLoader(ds, BATCH, shuffle=True, seed=1, drop_last=True)
        auged = dd.DeviceLoader(ds, BATCH, shuffle=True, seed=1, drop_last=True, augment=aug)
        nb = len(plain)

        def resident():
            for _ in range(nb):
                step(x, y)
            return nb * BATCH

        def fed(loader):
            k = 0
            for images, masks in data.DevicePrefetcher(loader, dev):
                if images.shape[0] == BATCH:
                    step(images, masks)
                    k += BATCH
            return k

        variants = {"step on resident data": resident, "DeviceLoader": lambda: fed(plain), "DeviceLoader + Augment": lambda: fed(auged),
                    "16 workers + pinned memory + DevicePrefetcher": lambda: fed(host16)}
        rates = {k: [] for k in variants}
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for k, fn in variants.items():
                t0 = time.perf_counter()
                done = fn()
                torch.cuda.synchronize()
                rates[k].append(done / (time.perf_counter() - t0))
        for k in variants:
            show(f"RobustUNet(64) training epoch at {size}^2, {nb} steps, {k}", rates[k], "img/s")


if __name__ == "__main__":
    main()
