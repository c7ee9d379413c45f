"""A decline of the device readers (reads.ReadsDeviceError, maf.MafDeviceError) that is raised after the upload must not keep the reader's
device tensors alive: a caller who keeps the error - `pytest.raises(...) as ex` does, and so does a log of failures - would otherwise
hold the file's bytes and every table on the device until a garbage collection breaks the traceback's cycle."""
import gc

import pytest
import torch

from gnnome_amd import maf, reads

pytestmark = pytest.mark.gpu

T = "strand=+ start=1 end=9 chr=2"
CASES = [   # (reader, file name, text, wanted names, keywords, the 1-based line named)
    ("reads", "x.fasta", f">a {T}\nACGT\nAC GT\n" + "ACGT" * 4096 + "\n", ["a", "b"], dict(titles=True), 3),
    ("reads", "x.fastq", "@z\n" + "ACGT" * 4096 + "\n+\n" + "I" * 16384 + f"\n@a {T}\nAC\tGT\n+\nIIII\n", ["a"], {}, 6),
    ("reads", "full.fasta", "".join(f">r{k}\nAC\n" for k in range(8)), [f"r{k}" for k in range(8)], dict(table_capacity=4), 0),
    ("maf", "x.maf", "a\ns ref 1 16384 + 99999 " + "ACGT" * 4096 + "\ns r 0 16383 + 16383 " + "ACGT" * 4096 + "\n", ["r"], {}, 3),
    ("maf", "full.maf", "".join(f"a\ns ref {k} 2 + 99 AC\ns r{k} 0 2 + 2 AC\n\n" for k in range(8)), [f"r{k}" for k in range(8)],
     dict(table_capacity=4), 0),
]


@pytest.mark.parametrize("reader,name,text,names,options,line", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_a_kept_decline_holds_no_device_memory(tmp_path, reader, name, text, names, options, line):
    path = tmp_path / name
    path.write_bytes(text.encode("ascii"))
    device = torch.device("cuda", 0)
    if reader == "reads":
        run, declined = (lambda: reads.read_reads_device(str(path), names, device=device, **options)), reads.ReadsDeviceError
    else:
        run, declined = (lambda: maf.read_maf_annotations(str(path), names, 5, parser="device", device=device, **options)), maf.MafDeviceError
    gc.collect()                      # earlier tests' garbage goes now, not between the two readings below
    gc.disable()
    try:
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(device)
        with pytest.raises(declined) as ex:
            run()
        assert ex.value.line == line
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated(device) == before      # with the error still in hand, and no collection having run
    finally:
        gc.enable()
