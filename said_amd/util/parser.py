"""Widely-used parsers (reference: said/util/parser.py)."""
from __future__ import annotations

from typing import Callable, List, TypeVar

T = TypeVar("T")


def parse_list(file_path: str, typecast_func: Callable[[str], T]) -> List[T]:
    """One item per line of the file, stripped and passed through typecast_func."""
    with open(file_path, "r") as f:
        return [typecast_func(line.strip()) for line in f.readlines()]
