"""The SAM file around the records DeviceEngine.sam_records / FmIndex.sam_records_raw make: the header lines and a writer.

The records themselves are formatted on the device (include/gdx_experimental.h "SAM records"); nothing here touches them."""
from __future__ import annotations


def _text(x) -> str:
    return x.decode() if isinstance(x, (bytes, bytearray)) else str(x)


def header(text_names, text_lengths, sort_order: str = "unsorted") -> bytes:
    """The @HD line and one @SQ line per text: `text_names` as the records' RNAME spell them (None: the decimal text ids, which is
    what the records hold when they were made without text names), `text_lengths` the texts' lengths in symbols."""
    lengths = [int(n) for n in text_lengths]
    names = [str(i) for i in range(len(lengths))] if text_names is None else [_text(x) for x in text_names]
    if len(names) != len(lengths):
        raise ValueError(f"{len(names)} text names for {len(lengths)} lengths")
    lines = [f"@HD\tVN:1.6\tSO:{sort_order}"] + [f"@SQ\tSN:{name}\tLN:{n}" for name, n in zip(names, lengths)]
    return ("\n".join(lines) + "\n").encode()


def write(path_or_file, records, text_names, text_lengths, sort_order: str = "unsorted") -> int:
    """Writes header(text_names, text_lengths) and then `records` -- the bytes of the record buffer (bytes, a numpy uint8 array or
    a torch uint8 tensor, which is copied to the host here) -- to a path or an open binary file.  -> the bytes written."""
    if hasattr(records, "detach"):
        records = records.detach().cpu().numpy()
    body = records.tobytes() if hasattr(records, "tobytes") else bytes(records)
    head = header(text_names, text_lengths, sort_order)
    if hasattr(path_or_file, "write"):
        path_or_file.write(head)
        path_or_file.write(body)
    else:
        with open(path_or_file, "wb") as f:
            f.write(head)
            f.write(body)
    return len(head) + len(body)
