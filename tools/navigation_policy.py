"""The small MLP behind the navigation fixtures' low-level policy archive, and the writer of the archive.

    PYTHONHASHSEED=0 python tools/navigation_policy.py <out.pt> <seed> <dim0> <dim1> ...

``LowLevelPolicy`` has the structure the reference's exporter writes (an ``actor`` Sequential, an Identity ``normalizer``,
``forward = actor(normalizer(x))``, isaaclab_rl/rsl_rl/exporter.py) around seeded default ``nn.Linear`` layers with ELU between them.
tools/gen_golden_navigation.py runs this file in a child interpreter with a fixed hash seed (TorchScript writes a module's constants
in set order) so that the committed archive is reproducible bit for bit."""

from __future__ import annotations

import sys

import torch


class LowLevelPolicy(torch.nn.Module):
    """The exporter's structure (``forward = actor(normalizer(x))``) around this project's own MLP."""

    def __init__(self, dims, seed: int):
        super().__init__()
        torch.manual_seed(seed)
        layers = []
        for i in range(len(dims) - 1):
            layers.append(torch.nn.Linear(dims[i], dims[i + 1]))
            if i + 2 < len(dims):
                layers.append(torch.nn.ELU())
        self.actor = torch.nn.Sequential(*layers)
        self.normalizer = torch.nn.Identity()
        self.requires_grad_(False)

    def forward(self, x):
        return self.actor(self.normalizer(x))

    def layers(self):
        return [(m.weight.detach().clone(), m.bias.detach().clone()) for m in self.actor if isinstance(m, torch.nn.Linear)]


def write_archive(module: LowLevelPolicy, path: str):
    """``torch.jit.save``, then the same records re-written as a plain stored zip with the one random record (the serialization id)
    fixed: the committed file is reproducible bit for bit, and ``torch.jit.load`` reads it like any archive."""
    import io
    import zipfile

    buf = io.BytesIO()
    torch.jit.save(torch.jit.script(module.eval()), buf)
    zin = zipfile.ZipFile(io.BytesIO(buf.getvalue()))
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as zout:
        for info in zin.infolist():
            data = b"0" * 40 if info.filename.endswith(".data/serialization_id") else zin.read(info)
            entry = zipfile.ZipInfo(info.filename, date_time=(1980, 1, 1, 0, 0, 0))
            entry.compress_type, entry.external_attr = zipfile.ZIP_STORED, 0
            zout.writestr(entry, data)


if __name__ == "__main__":
    write_archive(LowLevelPolicy([int(d) for d in sys.argv[3:]], int(sys.argv[2])), sys.argv[1])
