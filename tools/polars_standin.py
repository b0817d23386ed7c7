"""A stand-in for the few polars calls the reference's preprocess.py makes in `process_df` and `split_eventtable_in_chunks`, on numpy.
polars is not in the build image; `tools/make_goldens.py preprocess` installs this module under the name `polars` before it imports the
reference, so that the reference's own chunk cutting runs unmodified over it.  It is NOT polars: beside every call stands the polars
behaviour it takes the place of, and the generator chooses its inputs so that nothing this module has to invent (the order of ties in a
sort, how a text becomes a float) can reach an output.  Only what those two functions call exists here; anything else raises.

A frame is a dict of equally long numpy arrays (object arrays hold the texts); `from_table_text` builds one from an event table with the
column types `polars.read_csv(separator="\\t")` infers for such a table: Int64 for position / start_idx / end_idx, Float64 for
event_level_mean / event_stdv, Utf8 for read_name / model_kmer / samples."""
import numpy as np

Utf8 = "Utf8"
Float32 = np.float32


class Expr:
    """pl.col(name) and what process_df derives from it: a function of a frame's columns."""

    def __init__(self, fn, name):
        self.fn, self.name = fn, name

    def __ne__(self, other):                        # polars: Expr != literal -> a Boolean column, row by row
        return Expr(lambda cols: self.fn(cols) != other, self.name)

    def __sub__(self, other):                       # polars: Expr - Expr -> the difference row by row (Int64 - Int64 -> Int64)
        return Expr(lambda cols: self.fn(cols) - other.fn(cols), self.name)

    def alias(self, name):                          # polars: the same column under a new name
        return Expr(self.fn, name)

    def map_elements(self, fn, return_dtype=None):  # polars: the Python function applied to every value of the column, one by one
        def run(cols):
            out = np.empty(len(self.fn(cols)), object)
            out[:] = [fn(v) for v in self.fn(cols)]
            return out
        return Expr(run, self.name)


def col(name):
    return Expr(lambda cols: cols[name], name)


class _Str:
    def __init__(self, values):
        self.values = values

    def split(self, by):                            # polars: Series.str.split -> a List(Utf8) column, one list per row
        out = np.empty(len(self.values), object)
        out[:] = [v.split(by) for v in self.values]
        return Series(out)


class Series:
    def __init__(self, values):
        self.values = values

    @property
    def str(self):
        return _Str(self.values)

    def to_numpy(self):                             # polars: a 1-d array of the column's own type (Int64 -> int64, Float64 -> float64)
        return np.array(self.values)

    def to_list(self):                              # polars: a list of Python values
        return list(self.values)

    def explode(self):                              # polars: every list's items as rows of their own, in order
        items = [x for row in self.values for x in row]
        out = np.empty(len(items), object)
        out[:] = items
        return Series(out)

    def cast(self, dtype):
        # polars: Utf8 -> Float32 parses every text as a decimal number.  Here: text -> double -> fp32.  Whether polars rounds once or
        # twice is not known here; the generator only writes texts whose value is exact in fp32, where every parser agrees.
        assert dtype is Float32
        return Series(np.array([float(v) for v in self.values], np.float64).astype(np.float32))


class DataFrame:
    def __init__(self, columns):
        self.columns = dict(columns)
        assert len({len(v) for v in self.columns.values()}) == 1

    def __len__(self):
        return len(next(iter(self.columns.values())))

    def __getitem__(self, name):                    # polars: df["name"] -> the column as a Series
        return Series(self.columns[name])

    def _take(self, index):
        return DataFrame({k: v[index] for k, v in self.columns.items()})

    def partition_by(self, name):
        # polars: one frame per distinct value, the groups in order of first appearance (maintain_order=True is the default), the rows
        # of a group in their order in the frame.
        keys = self.columns[name]
        first = {}
        for i, v in enumerate(keys):
            first.setdefault(v, []).append(i)
        return [self._take(np.array(rows, np.int64)) for rows in first.values()]

    def sort(self, by):
        # polars: rows by the key, ascending; NO promise on the order of rows with equal keys (maintain_order=False is the default).
        # Here ties keep their order, which is this module's choice: the generator gives every row of a frame its own position, so
        # the reference's last sort, by position, decides the whole order whatever an earlier sort by the (constant) read_name did.
        (name,) = by
        return self._take(np.argsort(self.columns[name], kind="stable"))

    def filter(self, expr):                         # polars: the rows where the Boolean column is true, in their order
        return self._take(np.flatnonzero(expr.fn(self.columns)))

    def with_columns(self, expr):                   # polars: the frame with the expression's column added (or replaced) under its name
        cols = dict(self.columns)
        cols[expr.name] = expr.fn(self.columns)
        return DataFrame(cols)


def from_table_text(text):
    """An event table (tab separated, a header line) -> DataFrame.  The columns' types are those read_csv infers; event_stdv is parsed
    as a double, which is exact for the texts the generator writes."""
    lines = text.split("\n")
    head = lines[0].split("\t")
    rows = [line.split("\t") for line in lines[1:] if line]
    kinds = dict(read_name=str, position=np.int64, model_kmer=str, start_idx=np.int64, end_idx=np.int64, event_level_mean=np.float64,
                 event_stdv=np.float64, samples=str)
    cols = {}
    for c, name in enumerate(head):
        if kinds[name] is str:
            cols[name] = np.empty(len(rows), object)
            cols[name][:] = [r[c] for r in rows]
        else:
            cols[name] = np.array([kinds[name](r[c]) for r in rows], kinds[name])
    return DataFrame(cols)
