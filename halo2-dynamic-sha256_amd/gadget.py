"""Python view of the C++ gadget front-end (csrc/hsw_gadget.hpp): the same
names as the reference's `Sha256DynamicConfig` (src/lib.rs:38-369).  All logic
lives in libhsw.so; this file only marshals arguments."""
import ctypes as C

from . import _native as N


class AssignedHashResult:
    """lib.rs:31-36 on values."""

    def __init__(self, r, input_bytes):
        self.input_len = int(r.input_len)
        self._input_bytes = input_bytes          # bytes, or a callable fetching them on first use
        self.output_bytes = bytes(r.output_bytes)
        self.first_block = int(r.first_block)
        self.n_blocks = int(r.n_blocks)
        self.spread_cursor0 = int(r.spread_cursor0)
        self.num_round = int(r.num_round)
        self.target_round = int(r.target_round)
        # whole-digest contexts: where the sections of this digest start (cells), else 0
        for k in ("prologue_cell", "block_cell", "epilogue_cell", "end_cell",
                  "prologue_lookup", "block_lookup", "epilogue_lookup"):
            setattr(self, k, int(getattr(r, k)))


    @property
    def input_bytes(self):
        """assigned_input_bytes (lib.rs:170-173): the padded variable part, max_variable_byte_size bytes."""
        if callable(self._input_bytes):
            self._input_bytes = self._input_bytes()
        return self._input_bytes


class Sha256DynamicConfig:
    """configure (lib.rs:49-69) + new_context (lib.rs:351-360) in one object."""

    def __init__(self, engine, max_variable_byte_sizes, is_input_range_check=True, whole_digest=False, independent=False,
                 context_images=False, shared_context=False, n_contexts=None):
        """whole_digest: also emit the cells digest() itself allocates (lib.rs:122-178, 294-341;
        SURVEY 8 f4, assumption A4) -- needs an engine in HSW_MODE_HALO2_INTERNALS.
        independent: every digest is a synthesis of its own (HSW_GADGET_INDEPENDENT: K proofs in one launch).
        context_images: with independent, every proof gets a column image and lookup column of its own at the same
        Context origin (HSW_GADGET_CONTEXT_IMAGES; all max_variable_byte_sizes equal).
        shared_context: with whole_digest, every digest works on the same Context and the circuit may assign cells
        of its own between two digests (HSW_GADGET_SHARED_CONTEXT, set_digest_origin); layouts of up to
        HSW_GADGET_MAX_COLUMNS columns.
        n_contexts: a Context group (hsw_gadget_create_contexts) -- n_contexts proofs of one circuit whose digests
        max_variable_byte_sizes lists (ONE Context's), each laid out like a shared context, the layouts repeating
        like context images; whole_digest is implied, digest d of the pass is digest d % M of Context d // M."""
        self.engine = engine
        self.n_contexts = None if n_contexts is None else int(n_contexts)
        self.whole_digest = bool(whole_digest) or n_contexts is not None
        self.context_images = bool(context_images)
        self.lib = engine.lib
        self.max_variable_byte_sizes = list(max_variable_byte_sizes)
        arr = (C.c_size_t * max(len(self.max_variable_byte_sizes), 1))(*self.max_variable_byte_sizes)
        h = C.c_void_p()
        flags = ((N.HSW_GADGET_WHOLE_DIGEST if self.whole_digest else 0) |
                 (N.HSW_GADGET_INDEPENDENT if independent else 0) |
                 (N.HSW_GADGET_CONTEXT_IMAGES if context_images else 0) |
                 (N.HSW_GADGET_SHARED_CONTEXT if shared_context else 0))
        if n_contexts is not None:
            rc = self.lib.hsw_gadget_create_contexts(engine.h, arr, len(self.max_variable_byte_sizes), self.n_contexts,
                                                     1 if is_input_range_check else 0, flags, C.byref(h))
        else:
            rc = self.lib.hsw_gadget_create_ex(engine.h, arr, len(self.max_variable_byte_sizes),
                                               1 if is_input_range_check else 0, flags, C.byref(h))
        if rc != N.HSW_OK:
            raise N.HswError(rc, self.lib.hsw_last_error(engine.h).decode())
        self.h = h
        self._n = 0
        self._pending = []      # results whose input_bytes have not been fetched yet

    def _resolve_pending(self):
        for r in self._pending:
            r.input_bytes               # fetch while the gadget still holds them
        self._pending = []

    def close(self):
        if getattr(self, "h", None):
            self._resolve_pending()
            self.lib.hsw_gadget_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ok(self, rc):
        if rc != N.HSW_OK:
            raise N.HswError(rc, self.lib.hsw_last_error(self.engine.h).decode())

    def _input_bytes(self, idx):
        n = C.c_size_t()
        self._ok(self.lib.hsw_gadget_input_bytes(self.h, idx, None, 0, C.byref(n)))
        buf = (C.c_uint8 * max(n.value, 1))()
        self._ok(self.lib.hsw_gadget_input_bytes(self.h, idx, buf, n.value, None))
        return bytes(buf[: n.value])

    def digest(self, message: bytes, precomputed_input_len=None):
        """lib.rs:71-349; precomputed_input_len None == the reference's Option::None."""
        return self.digest_batch([message], [precomputed_input_len])[0]

    def digest_batch(self, messages, precomputed_input_lens=None):
        n = len(messages)
        keep = [bytes(m) for m in messages]
        bufs = [(C.c_uint8 * max(len(m), 1)).from_buffer_copy(m if m else b"\0") for m in keep]
        ptrs = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
        lens = (C.c_size_t * n)(*[len(m) for m in keep])
        pl = precomputed_input_lens or [None] * n
        pre = (C.c_size_t * n)(*[int(p or 0) for p in pl])
        res = (N.HashResult * n)()
        self._ok(self.lib.hsw_gadget_digest_batch(self.h, n, ptrs, lens, pre, res))
        base = self._n
        out = [AssignedHashResult(res[i], (lambda k=base + i: self._input_bytes(k))) for i in range(n)]
        self._n += n
        self._pending.extend(out)
        return out

    def digest_batch_device(self, inputs, precomputed_input_lens=None):
        """hsw_gadget_digest_batch_device: digest_batch for messages that already live in device memory.  Every
        input is a contiguous 1-D torch.uint8 device tensor (its data_ptr() and numel() are taken; the caller keeps
        it alive) or a (device_ptr, length) pair; lengths are host values.  The bytes must be complete before the
        call -- produced on the engine's stream, or synchronised -- and must not overlap what the gadget writes."""
        ptrs_, lens_ = self._device_inputs(inputs)
        n = len(ptrs_)
        ptrs = (C.c_void_p * max(n, 1))(*ptrs_)
        lens = (C.c_size_t * max(n, 1))(*lens_)
        pl = precomputed_input_lens or [None] * n
        pre = (C.c_size_t * max(n, 1))(*[int(p or 0) for p in pl])
        res = (N.HashResult * max(n, 1))()
        self._ok(self.lib.hsw_gadget_digest_batch_device(self.h, n, ptrs, lens, pre, res))
        return self._assigned(res, n)

    @staticmethod
    def _device_inputs(inputs):
        """(pointers, lengths) of device-fed inputs, checked in full before any call into the library."""
        ptrs_, lens_ = [], []
        for x in inputs:
            if isinstance(x, (tuple, list)):
                p, ln = x
                p, ln = int(p or 0), int(ln)
                if ln < 0 or (ln and not p):
                    raise ValueError("a (device_ptr, length) input needs a pointer for a non-zero length")
            else:
                import torch
                if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 or x.dim() != 1:
                    raise TypeError("inputs are 1-D torch.uint8 device tensors or (device_ptr, length) pairs")
                if not x.is_cuda or not x.is_contiguous():
                    raise ValueError("an input tensor must be contiguous and live on the device")
                p, ln = (int(x.data_ptr()) if x.numel() else 0), int(x.numel())
            ptrs_.append(p)
            lens_.append(ln)
        return ptrs_, lens_

    def _assigned(self, res, n):
        base = self._n
        out = [AssignedHashResult(res[i], (lambda k=base + i: self._input_bytes(k))) for i in range(n)]
        self._n += n
        self._pending.extend(out)
        return out

    def digest_levels_device(self, inputs, levels=None, outputs=None, precomputed_input_lens=None):
        """hsw_gadget_digest_levels_device: digest_batch_device for messages that depend on each other's digests.
        inputs as for digest_batch_device.  levels[i] (default: all 0) is message i's dependency level, in any order.
        outputs[i] is a contiguous 1-D torch.uint8 device tensor of 32 elements, an integer device pointer to 32
        writable bytes of any alignment, or None; digest i is written there, and a message may read what a message
        of a strictly lower level of the same call writes -- with no host read in between.  Overlapping outputs, and
        an input overlapping the output of a message not of a lower level, raise HswError (HSW_ERR_INVALID_ARG)."""
        ptrs_, lens_ = self._device_inputs(inputs)
        n = len(ptrs_)
        if levels is not None:
            levels = [int(v) for v in levels]
            if len(levels) != n or any(v < 0 or v > 0xffffffff for v in levels):
                raise ValueError("levels holds one non-negative 32-bit level per input")
        outs_ = None
        if outputs is not None:
            outputs = list(outputs)
            if len(outputs) != n:
                raise ValueError("outputs holds one entry (or None) per input")
            outs_ = []
            for x in outputs:
                if x is None:
                    p = 0
                elif hasattr(x, "data_ptr") or isinstance(x, bool) or not hasattr(x, "__index__"):
                    import torch
                    if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 or x.dim() != 1:
                        raise TypeError("outputs are 1-D torch.uint8 device tensors of 32 elements, device pointers or None")
                    if not x.is_cuda or not x.is_contiguous() or x.numel() != 32:
                        raise ValueError("an output tensor must hold 32 contiguous bytes on the device")
                    p = int(x.data_ptr())
                else:
                    p = int(x)
                    if p <= 0:
                        raise ValueError("an integer output is a non-null device pointer (None: no output)")
                outs_.append(p)
        if precomputed_input_lens is not None and len(precomputed_input_lens) != n:
            raise ValueError("precomputed_input_lens holds one entry (or None) per input")
        ptrs = (C.c_void_p * max(n, 1))(*ptrs_)
        lens = (C.c_size_t * max(n, 1))(*lens_)
        pl = precomputed_input_lens or [None] * n
        pre = (C.c_size_t * max(n, 1))(*[int(p or 0) for p in pl])
        lv = (C.c_uint32 * max(n, 1))(*levels) if levels is not None else None
        outs = (C.c_void_p * max(n, 1))(*outs_) if outs_ is not None else None
        res = (N.HashResult * max(n, 1))()
        self._ok(self.lib.hsw_gadget_digest_levels_device(self.h, n, ptrs, lens, pre, lv, outs, res))
        return self._assigned(res, n)

    def merkle_tree_device(self, leaves, nodes):
        """A binary Merkle tree over n = 2^d leaves in one digest_levels_device call (the gadget's next 2n - 1
        digests).  leaves: device inputs as for digest_batch_device; nodes: a contiguous 1-D torch.uint8 device tensor
        of 32 * (2n - 1) bytes.  Level 0, the leaf digests, fills nodes[0 : 32n]; every further level follows the one
        below it in memory; an inner message is the 64 bytes of its two children where they lie, never copied; the
        root is the last 32 bytes.  Returns the results, leaves first."""
        import torch
        leaves = list(leaves)
        n = len(leaves)
        if n < 1 or n & (n - 1):
            raise ValueError("merkle_tree_device takes a power-of-two number of leaves")
        if not isinstance(nodes, torch.Tensor) or nodes.dtype != torch.uint8 or nodes.dim() != 1:
            raise TypeError("nodes is a 1-D torch.uint8 device tensor")
        if not nodes.is_cuda or not nodes.is_contiguous() or nodes.numel() != 32 * (2 * n - 1):
            raise ValueError("nodes must hold 32 * (2n - 1) contiguous bytes on the device")
        base = int(nodes.data_ptr())
        inputs, levels = leaves, [0] * n
        below, width, level = 0, n, 0            # the level below: its first node and its width
        while width > 1:
            level += 1
            inputs = inputs + [(base + 32 * (below + 2 * j), 64) for j in range(width // 2)]
            levels += [level] * (width // 2)
            below, width = below + width, width // 2
        outputs = [base + 32 * k for k in range(2 * n - 1)]
        return self.digest_levels_device(inputs, levels, outputs)

    def set_columns(self, max_rows):
        """Lay the whole-digest stream out as FlexGate advice columns of max_rows rows (before the
        first digest).  Returns the number of columns."""
        n = C.c_uint64()
        self._ok(self.lib.hsw_gadget_set_columns(self.h, max_rows, C.byref(n)))
        return int(n.value)

    def set_origin(self, column=0, row=0, zero_cell_loaded=False, lookups_queued=0):
        """Where the caller's halo2-base Context stands when the gadget takes over (hsw_gadget_set_origin):
        ctx.advice_alloc[0] = (column, row), ctx.zero_cell.is_some(), ctx.cells_to_lookup.len()."""
        self._ok(self.lib.hsw_gadget_set_origin(self.h, column, row, 1 if zero_cell_loaded else 0, lookups_queued))

    def set_digest_origin(self, h, column, row, lookups_queued):
        """Where the shared Context stands just before digest h (hsw_gadget_set_digest_origin): ctx.advice_alloc[0] =
        (column, row) and ctx.cells_to_lookup.len() after the circuit's own cells since digest h-1."""
        self._ok(self.lib.hsw_gadget_set_digest_origin(self.h, h, column, row, lookups_queued))

    def bind_region(self, columns, column_pitch=0, columns_capacity=0, lookup=None, lookup_capacity=0, chip_dense=None,
                    chip_spread=None, chip_col_stride=0, chip_rows_capacity=0, context_pitch=0, lookup_pitch=0,
                    chip_context_pitch=0):
        """hsw_gadget_bind_region: write the region straight into device columns the caller owns.  columns, lookup,
        chip_dense, chip_spread: torch tensors (their data_ptr is taken; the caller keeps them alive and disjoint) or
        raw device pointers; pitches and capacities in cells.  bind_region(None): back to library-owned buffers."""
        if columns is None:
            self._ok(self.lib.hsw_gadget_bind_region(self.h, None))
            self._bound = None
            self._column_ptrs = self._lookup_ptrs = self._chip_ptrs = None
            return

        def ptr(x):
            return int(x.data_ptr()) if hasattr(x, "data_ptr") else int(x or 0)
        b = N.RegionBinding(ptr(columns), column_pitch, columns_capacity, context_pitch, ptr(lookup), lookup_capacity, lookup_pitch,
                            ptr(chip_dense), ptr(chip_spread), chip_col_stride, chip_rows_capacity, chip_context_pitch)
        self._ok(self.lib.hsw_gadget_bind_region(self.h, C.byref(b)))
        self._bound = (columns, lookup, chip_dense, chip_spread)      # keeps tensors alive while they are bound
        self._column_ptrs = self._lookup_ptrs = self._chip_ptrs = None

    def bind_columns(self, column_ptrs, column_pitch, columns_capacity, lookup=None, lookup_capacity=0, chip_dense=None,
                     chip_spread=None, chip_col_stride=0, chip_rows_capacity=0, lookup_pitch=0, chip_context_pitch=0,
                     lookup_ptrs=None, chip_dense_ptrs=None, chip_spread_ptrs=None):
        """hsw_gadget_bind_columns: like bind_region, but every FlexGate image column is an allocation of its own.
        column_ptrs[c * columns_capacity + k]: torch tensor or raw device pointer of row 0 of image column k of proof c
        (K * columns_capacity entries; the caller keeps them alive); column_pitch: cells each column holds.  Lookup and
        chip areas as in bind_region -- or, with lookup_ptrs= (K entries: proof c's lookup-advice column) and / or
        chip_dense_ptrs= and chip_spread_ptrs= (K * ncols entries each: [c * ncols + k] = chip column k of proof c), by
        pointer table too (hsw_gadget_bind_column_tables; tensors or integers like column_ptrs, lookup_capacity /
        chip_rows_capacity = what each allocation holds).  bind_region(None) unbinds."""
        def ptr(x):
            return int(x.data_ptr()) if hasattr(x, "data_ptr") else int(x or 0)

        def table(xs):
            v = [ptr(x) for x in xs]
            return v, (C.c_void_p * max(len(v), 1))(*v)
        ptrs, arr = table(column_ptrs)
        b = N.RegionBinding(None, column_pitch, columns_capacity, 0, ptr(lookup), lookup_capacity, lookup_pitch,
                            ptr(chip_dense), ptr(chip_spread), chip_col_stride, chip_rows_capacity, chip_context_pitch)
        lks = cds = css = None
        if lookup_ptrs is None and chip_dense_ptrs is None and chip_spread_ptrs is None:
            self._ok(self.lib.hsw_gadget_bind_columns(self.h, C.byref(b), arr, len(ptrs)))
        else:
            t = N.ColumnTables(C.cast(arr, C.POINTER(C.c_void_p)), len(ptrs), None, 0, None, None, 0)
            keep = [arr]
            if lookup_ptrs is not None:
                lks, a = table(lookup_ptrs)
                t.d_lookup_ptrs, t.n_lookup_ptrs = C.cast(a, C.POINTER(C.c_void_p)), len(lks)
                keep.append(a)
            if chip_dense_ptrs is not None:
                cds, a = table(chip_dense_ptrs)
                t.d_chip_dense_ptrs, t.n_chip_ptrs = C.cast(a, C.POINTER(C.c_void_p)), len(cds)
                keep.append(a)
            if chip_spread_ptrs is not None:
                css, a = table(chip_spread_ptrs)
                t.d_chip_spread_ptrs, t.n_chip_ptrs = C.cast(a, C.POINTER(C.c_void_p)), max(len(css), int(t.n_chip_ptrs))
                keep.append(a)
            self._ok(self.lib.hsw_gadget_bind_column_tables(self.h, C.byref(b), C.byref(t)))
        self._bound = (list(column_ptrs), lookup, chip_dense, chip_spread, lookup_ptrs, chip_dense_ptrs, chip_spread_ptrs)
        self._column_ptrs = ptrs
        self._lookup_ptrs = lks
        self._chip_ptrs = (cds, css) if cds is not None and css is not None else None

    def _unbound_only(self, what):
        """The numpy conveniences size their host buffers for library-owned geometry; a bound gadget's host layout
        follows the caller's pitches: call hsw_gadget_download_region / hsw_gadget_replay_region with buffers of
        that geometry (region_binding())."""
        if getattr(self, "_bound", None) is not None:
            raise N.HswError(N.HSW_ERR_UNSUPPORTED, what + "(): bound region -- pass host buffers laid out like the binding to the C call")

    def region_binding(self):
        """hsw_gadget_region_binding: the geometry in force (also when library-owned)."""
        b = N.RegionBinding()
        self._ok(self.lib.hsw_gadget_region_binding(self.h, C.byref(b)))
        return b

    def reset(self):
        """Next synthesis pass: all cursors back to their start, buffers and layout kept
        (the reference clones the config per synthesis, lib.rs:440)."""
        self._resolve_pending()
        self._ok(self.lib.hsw_gadget_reset(self.h))
        self._n = 0

    def _image_shape(self, v):
        """Shape of the gate image: (columns, max_rows), or (K, columns, max_rows) with context images."""
        cr = (int(v.columns), int(v.max_rows))
        if self.n_contexts is not None:
            return (self.n_contexts,) + cr
        return (len(self.max_variable_byte_sizes),) + cr if self.context_images else cr

    def download_region(self, pinned=True):
        """hsw_gadget_download_region into (pinned) host arrays: dict of numpy uint64 arrays shaped like
        streams() -- gate (columns, max_rows, 4) or (cells, 4); lookup; dense / spread (ncols, stride, 4)."""
        import numpy as np
        self._unbound_only("download_region")
        v = self.view()
        ncols = self.engine.ncols
        img = self.whole_digest and int(v.max_rows)
        n_gate = int(np.prod(self._image_shape(v))) if img else (
            int(v.gate_cells) if self.whole_digest else int(v.blocks_done) * self.engine.G)
        stride = int(v.chip_col_stride)

        def buf(cells):
            if pinned:
                return self.engine.host_empty((max(cells, 1), 4))
            return np.zeros((max(cells, 1), 4), dtype=np.uint64)
        gate, dense, spread = buf(n_gate), buf(ncols * stride), buf(ncols * stride)
        lookup = buf(int(v.lookup_cells)) if self.whole_digest else None
        if img:
            gate[:] = 0                                    # unassigned tail rows of a column stay zero
        dst = N.RegionHost(gate.ctypes.data, lookup.ctypes.data if lookup is not None else None,
                           dense.ctypes.data, spread.ctypes.data)
        self._ok(self.lib.hsw_gadget_download_region(self.h, C.byref(dst)))
        rows = (int(v.num_limb_sum) + ncols - 1) // ncols
        out = dict(gate=gate[:n_gate].reshape(self._image_shape(v) + (4,)) if img else gate[:n_gate],
                   dense=dense.reshape(ncols, stride, 4)[:, :rows], spread=spread.reshape(ncols, stride, 4)[:, :rows],
                   rows=rows)
        if lookup is not None:
            out["lookup"] = lookup[: int(v.lookup_cells)]
        return out

    def place(self, candidates=3):
        """hsw_gadget_place: try `candidates` allocations of the chip columns, keep the one the gadget's own batch
        runs fastest on (fresh or reset gadget).  Returns (batch ms of every candidate, index kept)."""
        ms = (C.c_float * candidates)()
        kept = C.c_uint()
        self._ok(self.lib.hsw_gadget_place(self.h, candidates, ms, C.byref(kept)))
        return [float(x) for x in ms], int(kept.value)

    def download_region_distinct(self, threads=8, bufs=None):
        """Distinct-value delivery: only the new witnesses cross PCIe (hsw_gadget_download_region_distinct into
        pinned memory), the image is rebuilt on the host (hsw_gadget_replay_region).  Returns the same dict as
        download_region plus "distinct" (n, 4) and "bufs" (pass back in to reuse the host buffers)."""
        import numpy as np
        self._unbound_only("download_region_distinct")
        tape = N.RegionTape()
        self._ok(self.lib.hsw_gadget_region_tape(self.h, C.byref(tape)))
        v = self.view()
        ncols = self.engine.ncols
        img = int(v.max_rows)
        n_gate = int(np.prod(self._image_shape(v))) if img else int(v.gate_cells)
        stride = int(v.chip_col_stride)
        if bufs is None:          # sized for the whole gadget, so that they can be reused as more digests are assigned
            bufs = dict(distinct=self.engine.host_empty((max(int(tape.distinct_capacity), 1), 4)),
                        gate=np.zeros((max(n_gate if img else int(v.gate_capacity), 1), 4), dtype=np.uint64), lookup=np.zeros((max(int(v.lookup_capacity), 1), 4), dtype=np.uint64),
                        dense=np.zeros((ncols * stride, 4), dtype=np.uint64), spread=np.zeros((ncols * stride, 4), dtype=np.uint64))
        n = C.c_size_t()
        self._ok(self.lib.hsw_gadget_download_region_distinct(self.h, bufs["distinct"].ctypes.data, bufs["distinct"].shape[0], C.byref(n)))
        dst = N.RegionHost(bufs["gate"].ctypes.data, bufs["lookup"].ctypes.data, bufs["dense"].ctypes.data, bufs["spread"].ctypes.data)
        self._ok(self.lib.hsw_gadget_replay_region(self.h, bufs["distinct"].ctypes.data, C.byref(dst), threads))
        rows = (int(v.num_limb_sum) + ncols - 1) // ncols
        return dict(gate=bufs["gate"][:n_gate].reshape(self._image_shape(v) + (4,)) if img else bufs["gate"][:n_gate],
                    lookup=bufs["lookup"][: int(v.lookup_cells)], dense=bufs["dense"].reshape(ncols, stride, 4)[:, :rows],
                    spread=bufs["spread"].reshape(ncols, stride, 4)[:, :rows], rows=rows, distinct=bufs["distinct"][: n.value],
                    n_distinct=int(n.value), bufs=bufs)

    def download_region_compact(self, bufs=None):
        """hsw_gadget_download_region_compact into pinned host arrays: 8-byte cells + the side list of the cells
        wider than 64 bits.  Returns (bufs, n_wide); pass `bufs` back in to reuse the buffers.  widen() rebuilds
        the 32-byte streams on the host (hsw_region_widen)."""
        import numpy as np
        v = self.view()
        ncols = self.engine.ncols
        img = self.whole_digest and int(v.max_rows)
        n_gate = int(v.max_rows) * int(v.columns) if img else (
            int(v.gate_cells) if self.whole_digest else int(v.blocks_done) * self.engine.G)
        stride = int(v.chip_col_stride)
        if bufs is None:
            cap = 300 * max(int(v.capacity_blocks), 1) + 4096
            bufs = dict(gate=self.engine.host_empty((max(n_gate, 1),)), dense=self.engine.host_empty((ncols * stride,)),
                        spread=self.engine.host_empty((ncols * stride,)), wide=self.engine.host_empty((cap, 6)), cap=cap)
            bufs["lookup"] = self.engine.host_empty((max(int(v.lookup_cells), 1),)) if self.whole_digest else None
            if img:
                bufs["gate"][:] = 0
        dst = N.RegionCompact(bufs["gate"].ctypes.data, bufs["lookup"].ctypes.data if bufs["lookup"] is not None else None,
                              bufs["dense"].ctypes.data, bufs["spread"].ctypes.data, bufs["wide"].ctypes.data, bufs["cap"], 0)
        self._ok(self.lib.hsw_gadget_download_region_compact(self.h, C.byref(dst)))
        return bufs, int(dst.n_wide)

    def widen(self, compact, stream_id, wide, n_wide):
        """hsw_region_widen: one stream's 32-byte canonical cells from its compact form + the side list."""
        import numpy as np
        compact = np.ascontiguousarray(compact, dtype=np.uint64).reshape(-1)
        out = np.zeros((compact.size, 4), dtype=np.uint64)
        self._ok(self.lib.hsw_region_widen(compact.ctypes.data, compact.size, stream_id, wide.ctypes.data, n_wide,
                                           out.ctypes.data))
        return out

    def verify(self):
        """hsw_gadget_verify: everything written so far against the constraint system, on the device."""
        rep = N.VerifyReport()
        self._ok(self.lib.hsw_gadget_verify(self.h, C.byref(rep)))
        return dict(violations=int(rep.violations), checks=int(rep.checks), first_block=int(rep.first_block),
                    first_cell=int(rep.first_cell), first_class=N.VerifyReport.CLASSES.get(int(rep.first_class)),
                    kernel_ms=float(rep.kernel_ms))

    def ties(self):
        """hsw_gadget_ties: the digest-to-digest copy constraints of the pass -- (ties, prefix_bytes_untied), ties a
        numpy structured array (src_hash, dst_hash, src_byte, dst_byte, src_cell, dst_cell) in (dst_hash, dst_byte)
        order: the circuit adds constrain_equal(src_cell, dst_cell) for each."""
        import numpy as np
        dt = np.dtype([("src_hash", "<u8"), ("dst_hash", "<u8"), ("src_byte", "<u4"), ("dst_byte", "<u4"),
                       ("src_cell", "<u8"), ("dst_cell", "<u8")])
        n, pre = C.c_size_t(), C.c_uint64()
        self._ok(self.lib.hsw_gadget_ties(self.h, None, 0, C.byref(n), C.byref(pre)))
        out = np.zeros(n.value, dtype=dt)
        if n.value:
            self._ok(self.lib.hsw_gadget_ties(self.h, out.ctypes.data_as(C.POINTER(N.CellTie)), n.value, None, None))
        return out, int(pre.value)

    def cell_address(self, cell):
        """hsw_gadget_cell_address: device address of a gate-stream cell in the layout and binding in force."""
        p = C.c_void_p()
        self._ok(self.lib.hsw_gadget_cell_address(self.h, int(cell), C.byref(p)))
        return int(p.value or 0)

    @staticmethod
    def _tie_report(rep):
        return dict(violations=int(rep.violations), checks=int(rep.checks), first=int(rep.first), kernel_ms=float(rep.kernel_ms))

    def verify_ties(self):
        """hsw_gadget_verify_ties: every recorded tie, cell against cell on the device."""
        rep = N.TieReport()
        self._ok(self.lib.hsw_gadget_verify_ties(self.h, C.byref(rep)))
        return self._tie_report(rep)

    def verify_equal(self, cells_a, cells_b):
        """hsw_gadget_verify_equal: the caller's own constrain_equal pairs (gate-stream cells), compared as stored."""
        a, b = [int(x) for x in cells_a], [int(x) for x in cells_b]
        if len(a) != len(b):
            raise ValueError("verify_equal takes as many cells on one side as on the other")
        n = len(a)
        rep = N.TieReport()
        self._ok(self.lib.hsw_gadget_verify_equal(self.h, (C.c_uint64 * max(n, 1))(*a), (C.c_uint64 * max(n, 1))(*b), n, C.byref(rep)))
        return self._tie_report(rep)

    def lookup_runs(self):
        """hsw_gadget_lookup_runs: the lookup entries the digests of this pass have written, as runs of device cells --
        a list of dicts (context, table, column, first, n, d_cells, d_spread) in (context, table, column, first) order;
        table is HSW_LOOKUP_RANGE (lookup-advice column) or HSW_LOOKUP_SPREAD (chip column `column`)."""
        n = C.c_size_t()
        self._ok(self.lib.hsw_gadget_lookup_runs(self.h, None, 0, C.byref(n)))
        out = (N.LookupRun * max(n.value, 1))()
        if n.value:
            self._ok(self.lib.hsw_gadget_lookup_runs(self.h, out, n.value, None))
        return [dict(context=int(r.context), table=int(r.table), column=int(r.column), first=int(r.first), n=int(r.n),
                     d_cells=int(r.d_cells or 0), d_spread=int(r.d_spread or 0)) for r in out[: n.value]]

    def _lookup_contexts(self):
        return self.n_contexts if self.n_contexts is not None else len(self.max_variable_byte_sizes) if self.context_images else 1

    def lookup_multiplicities(self, range=True, spread=True, out_range=None, out_spread=None, accumulate=False):
        """hsw_gadget_lookup_multiplicities: how often every row of the 2^16-row range table and of the
        2^num_bits_lookup-row spread table is used by every proof of the pass, counted on the device.  Returns
        (range, spread, report): two int32 device tensors of shape (contexts, pitch) -- None for a table not asked for
        -- and the report as a dict.  out_range / out_spread: the caller's own tensors (contiguous int32 on the
        engine's device, (contexts, pitch) with pitch >= the table size), counted into; with accumulate the counters
        grow instead of being zeroed first.  A prover adds usable_rows - entries to row 0 of each table itself."""
        import torch
        k, dev = self._lookup_contexts(), self.engine.device
        want = (("range", range, out_range, 1 << 16), ("spread", spread, out_spread, 1 << int(self.engine.shape.num_bits_lookup)))
        if not (range or spread):
            raise ValueError("lookup_multiplicities: neither table asked for")
        tensors = []
        for name, on, t, rows in want:                     # everything checked before the library is called
            if not on:
                if t is not None:
                    raise ValueError("out_%s given for a table that is not asked for" % name)
                tensors.append(None)
                continue
            if t is None:
                if accumulate:
                    raise ValueError("accumulate needs the caller's own out_%s" % name)
                tensors.append((name, rows))
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
                raise ValueError("out_%s must be an int32 tensor" % name)
            if t.device != dev:
                raise ValueError("out_%s must live on %s" % (name, dev))
            if t.dim() != 2 or t.shape[0] != k or t.shape[1] < rows or not t.is_contiguous():
                raise ValueError("out_%s must be contiguous, of shape (%d, pitch >= %d)" % (name, k, rows))
            tensors.append(t)
        tensors = [torch.zeros((k, t[1]), dtype=torch.int32, device=dev) if isinstance(t, tuple) else t for t in tensors]
        r, s = tensors
        args = N.LookupCounts(r.data_ptr() if r is not None else None, s.data_ptr() if s is not None else None,
                              r.shape[1] if r is not None else 0, s.shape[1] if s is not None else 0,
                              N.HSW_LOOKUP_ACCUMULATE if accumulate else 0, 0)
        rep = N.LookupReport()
        torch.cuda.synchronize(dev)                        # the tensors were made on torch's stream, the count runs on the engine's
        self._ok(self.lib.hsw_gadget_lookup_multiplicities(self.h, C.byref(args), C.byref(rep)))
        return r, s, dict(range_entries=int(rep.range_entries), spread_entries=int(rep.spread_entries),
                          not_in_table=int(rep.not_in_table), first_context=int(rep.first_context), first_entry=int(rep.first_entry),
                          first_table=int(rep.first_table), first_column=int(rep.first_column), kernel_ms=float(rep.kernel_ms))

    def lookup_permuted(self, table, usable_rows, thetas=None, m=None, out_input=None, out_table=None, theta_on_spread=False):
        """hsw_gadget_lookup_permuted: halo2's permuted lookup columns A' and S' of every argument of `table`
        (HSW_LOOKUP_RANGE: one argument per proof; HSW_LOOKUP_SPREAD: one per proof and chip column), written on the
        device.  Returns (input, table, m, report): two uint64 device tensors of shape (arguments, usable_rows, 4), the
        int32 multiplicities (arguments, pitch) and the report as a dict.  thetas (SPREAD): one field element per proof
        AS STORED, i.e. in the representation of the cells (Montgomery cells: theta * 2^256 mod p) -- Python ints below p
        or a (contexts, 4) uint64 numpy array / tensor of limbs.  m: the caller's own multiplicities, a contiguous
        int32 tensor (arguments, pitch >= T) on the engine's device (HSW_PERMUTED_GIVEN_M); None: counted from the
        pass.  out_input / out_table: the caller's own contiguous uint64 tensors of shape (arguments, rows >=
        usable_rows, 4); rows from usable_rows on are never written.  report["written"] == 0: the device refused (an
        entry that is no table row, multiplicities beyond usable_rows) and stored nothing."""
        import numpy as np
        import torch
        dev = self.engine.device
        spread = table == N.HSW_LOOKUP_SPREAD
        if table not in (N.HSW_LOOKUP_RANGE, N.HSW_LOOKUP_SPREAD):
            raise ValueError("lookup_permuted: table must be HSW_LOOKUP_RANGE or HSW_LOOKUP_SPREAD")
        k = self._lookup_contexts()
        n_args = k * int(self.engine.shape.num_advice_columns) if spread else k
        rows = 1 << int(self.engine.shape.num_bits_lookup) if spread else 1 << 16
        u = int(usable_rows)
        if u < rows:
            raise ValueError("usable_rows must be at least the table size %d" % rows)
        cols = []
        for name, t in (("out_input", out_input), ("out_table", out_table)):
            if t is None:
                t = torch.zeros((n_args, u, 4), dtype=torch.uint64, device=dev)
            elif not isinstance(t, torch.Tensor) or t.dtype != torch.uint64 or t.device != dev:
                raise ValueError("%s must be a uint64 tensor on %s" % (name, dev))
            elif t.dim() != 3 or t.shape[0] != n_args or t.shape[1] < u or t.shape[2] != 4 or not t.is_contiguous():
                raise ValueError("%s must be contiguous, of shape (%d, rows >= %d, 4)" % (name, n_args, u))
            cols.append(t)
        if m is not None:
            if not isinstance(m, torch.Tensor) or m.dtype != torch.int32 or m.device != dev:
                raise ValueError("m must be an int32 tensor on %s" % (dev,))
            if m.dim() != 2 or m.shape[0] != n_args or m.shape[1] < rows or not m.is_contiguous():
                raise ValueError("m must be contiguous, of shape (%d, pitch >= %d)" % (n_args, rows))
        theta_buf = None
        if spread:
            if thetas is None:
                raise ValueError("the spread argument needs one theta per proof")
            if isinstance(thetas, torch.Tensor):
                thetas = thetas.cpu().numpy()
            if isinstance(thetas, np.ndarray):
                theta_buf = np.ascontiguousarray(thetas, dtype=np.uint64)
            else:
                theta_buf = np.array([[(int(v) >> (64 * i)) & (2**64 - 1) for i in range(4)] for v in thetas], dtype=np.uint64)
            if theta_buf.shape != (k, 4):
                raise ValueError("thetas: one field element (4 x uint64) per proof, %d of them" % k)
        elif thetas is not None:
            raise ValueError("thetas given for the range argument")
        counts = m if m is not None else torch.zeros((n_args, rows), dtype=torch.int32, device=dev)
        ptrs = [(C.c_void_p * n_args)(*[t.data_ptr() + a * t.shape[1] * 32 for a in range(n_args)]) for t in cols]
        flags = (N.HSW_PERMUTED_GIVEN_M if m is not None else 0) | (N.HSW_PERMUTED_THETA_ON_SPREAD if theta_on_spread else 0)
        args = N.LookupPermuted(table, flags, u, n_args, ptrs[0], ptrs[1], theta_buf.ctypes.data if theta_buf is not None else None,
                                counts.data_ptr(), counts.shape[1])
        rep = N.PermutedReport()
        torch.cuda.synchronize(dev)                        # the tensors were made on torch's stream, the call runs on the engine's
        self._ok(self.lib.hsw_gadget_lookup_permuted(self.h, C.byref(args), C.byref(rep)))
        return cols[0], cols[1], counts, {f[0]: getattr(rep, f[0]) for f in N.PermutedReport._fields_ if f[0] != "reserved_"}

    def lookup_product(self, table, usable_rows, betas, gammas, inputs, permuted_input, permuted_table, thetas=None,
                       inputs_spread=None, input_rows=None, out=None, theta_on_spread=False):
        """hsw_gadget_lookup_product: the grand-product column Z of every argument of `table`, written on the device:
        Z[0] = 1, Z[i+1] = Z[i] (A[i] + beta)(S[i] + gamma) / ((A'[i] + beta)(S'[i] + gamma)).  Returns (z, status,
        report): a uint64 device tensor (arguments, usable_rows + 1, 4), the uint32 numpy status array (HSW_PRODUCT_*
        bits per argument) and the report as a dict.  inputs (RANGE: the lookup-advice column; SPREAD: the dense
        column), inputs_spread (SPREAD only), permuted_input, permuted_table: either a contiguous uint64 tensor
        (arguments, rows, 4) on the engine's device or a sequence of `arguments` device addresses (ints, 16-byte
        aligned).  input_rows: per argument, the rows of its input that are assigned (the rest count as 0 and are not
        read); None: all usable_rows.  betas, gammas, thetas (SPREAD only): one field element per proof AS STORED, as
        lookup_permuted takes its thetas.  out: the caller's own contiguous uint64 tensor (arguments, rows >=
        usable_rows + 1, 4); rows beyond usable_rows are never written.  A refused argument (status & 6) is not written."""
        import numpy as np
        import torch
        dev = self.engine.device
        spread = table == N.HSW_LOOKUP_SPREAD
        if table not in (N.HSW_LOOKUP_RANGE, N.HSW_LOOKUP_SPREAD):
            raise ValueError("lookup_product: table must be HSW_LOOKUP_RANGE or HSW_LOOKUP_SPREAD")
        k = self._lookup_contexts()
        n_args = k * int(self.engine.shape.num_advice_columns) if spread else k
        rows = 1 << int(self.engine.shape.num_bits_lookup) if spread else 1 << 16
        u = int(usable_rows)
        if u < rows or u > 1 << 31:
            raise ValueError("usable_rows must be at least the table size %d and at most 2^31" % rows)
        if input_rows is None:
            in_rows = [u] * n_args
        else:
            in_rows = [int(r) for r in input_rows]
            if len(in_rows) != n_args or any(r < 0 or r > u for r in in_rows):
                raise ValueError("input_rows: %d values between 0 and usable_rows" % n_args)
        if spread != (inputs_spread is not None):
            raise ValueError("inputs_spread is the spread argument's (and required there)")

        def pointers(name, t, need):
            if isinstance(t, torch.Tensor):
                if t.dtype != torch.uint64 or t.device != dev:
                    raise ValueError("%s must be a uint64 tensor on %s" % (name, dev))
                if t.dim() != 3 or t.shape[0] != n_args or t.shape[1] < max(need) or t.shape[2] != 4 or not t.is_contiguous():
                    raise ValueError("%s must be contiguous, of shape (%d, rows >= %d, 4)" % (name, n_args, max(need)))
                return [t.data_ptr() + a * t.shape[1] * 32 for a in range(n_args)]
            ptrs = [int(p) for p in t]
            if len(ptrs) != n_args or any(p == 0 or p % 16 for p in ptrs):
                raise ValueError("%s: %d device addresses, 16-byte aligned" % (name, n_args))
            return ptrs

        cols = [pointers("inputs", inputs, in_rows)]
        cols.append(pointers("inputs_spread", inputs_spread, in_rows) if spread else None)
        cols.append(pointers("permuted_input", permuted_input, [u]))
        cols.append(pointers("permuted_table", permuted_table, [u]))
        if out is None:
            out = torch.zeros((n_args, u + 1, 4), dtype=torch.uint64, device=dev)
        elif not isinstance(out, torch.Tensor):
            raise ValueError("out must be a uint64 tensor on %s" % (dev,))
        cols.append(pointers("out", out, [u + 1]))

        def challenges(name, v):
            if v is None:
                raise ValueError("%s: one field element per proof" % name)
            if isinstance(v, torch.Tensor):
                v = v.cpu().numpy()
            if isinstance(v, np.ndarray):
                buf = np.ascontiguousarray(v, dtype=np.uint64)
            else:
                buf = np.array([[(int(x) >> (64 * i)) & (2**64 - 1) for i in range(4)] for x in v], dtype=np.uint64)
            if buf.shape != (k, 4):
                raise ValueError("%s: one field element (4 x uint64) per proof, %d of them" % (name, k))
            return buf

        b_buf, g_buf = challenges("betas", betas), challenges("gammas", gammas)
        if spread:
            t_buf = challenges("thetas", thetas)
        elif thetas is not None:
            raise ValueError("thetas given for the range argument")
        else:
            t_buf = None
        arr = [(C.c_void_p * n_args)(*c) if c is not None else None for c in cols]
        status = np.zeros(n_args, dtype=np.uint32)
        args = N.LookupProduct(table, N.HSW_PERMUTED_THETA_ON_SPREAD if theta_on_spread else 0, u, n_args, arr[0], arr[1],
                               (C.c_uint64 * n_args)(*in_rows), arr[2], arr[3], arr[4],
                               t_buf.ctypes.data if t_buf is not None else None, b_buf.ctypes.data, g_buf.ctypes.data,
                               status.ctypes.data_as(C.POINTER(C.c_uint32)))
        rep = N.ProductReport()
        torch.cuda.synchronize(dev)                        # the tensors were made on torch's stream, the call runs on the engine's
        self._ok(self.lib.hsw_gadget_lookup_product(self.h, C.byref(args), C.byref(rep)))
        return out, status, {f[0]: getattr(rep, f[0]) for f in N.ProductReport._fields_ if f[0] != "reserved_"}

    def permutation_product(self, usable_rows, chunk_columns, betas, gammas, omega, delta, columns, sigmas, column_rows=None,
                            out=None):
        """hsw_gadget_permutation_product: the permutation argument's grand products of every proof, written on the
        device: per chunk s of chunk_columns columns Z_s[i+1] = Z_s[i] prod_j (v_j[i] + beta delta^j omega^i + gamma) /
        prod_j (v_j[i] + beta sigma_j[i] + gamma), Z_0[0] = 1, Z_s[0] = Z_{s-1}[usable_rows].  Returns (z, status,
        report): a uint64 device tensor (proofs, S, usable_rows + 1, 4), the uint32 numpy status array (HSW_PRODUCT_*
        bits per proof) and the report as a dict.  sigmas: the m permutation columns of the key, shared by the proofs: a
        contiguous uint64 tensor (m, rows >= usable_rows, 4) on the engine's device or a sequence of m device addresses
        (ints, 16-byte aligned).  columns: the value columns in the permutation's order: a contiguous uint64 tensor
        (proofs, m, rows, 4) or a sequence of proofs * m device addresses, [c * m + j].  column_rows: proofs * m values,
        the rows of each column that are assigned (the rest count as 0 and are not read); None: all usable_rows.
        betas, gammas: one field element per proof AS STORED, as lookup_product takes them; omega, delta: one element
        each, as stored.  out: the caller's own contiguous uint64 tensor (proofs, S, rows >= usable_rows + 1, 4); rows
        beyond usable_rows are never written.  A refused proof (status & 6) is not written."""
        import numpy as np
        import torch
        dev = self.engine.device
        k, u, chunk = self._lookup_contexts(), int(usable_rows), int(chunk_columns)
        if u < 1 or u > 1 << 31:
            raise ValueError("usable_rows must be at least 1 and at most 2^31")
        if chunk < 1 or chunk > 0xffffffff:
            raise ValueError("chunk_columns must be at least 1")

        def pointers(name, t, lead, need):
            """device addresses of the prod(lead) columns of t, which must hold `need` rows"""
            n = int(np.prod(lead))
            if isinstance(t, torch.Tensor):
                if t.dtype != torch.uint64 or t.device != dev:
                    raise ValueError("%s must be a uint64 tensor on %s" % (name, dev))
                if t.dim() != len(lead) + 2 or tuple(t.shape[:len(lead)]) != tuple(lead) or t.shape[-2] < need or t.shape[-1] != 4 or not t.is_contiguous():
                    raise ValueError("%s must be contiguous, of shape (%s, rows >= %d, 4)" % (name, ", ".join(map(str, lead)), need))
                return [t.data_ptr() + a * t.shape[-2] * 32 for a in range(n)]
            ptrs = [int(p) for p in t]
            if len(ptrs) != n or any(p == 0 or p % 16 for p in ptrs):
                raise ValueError("%s: %d device addresses, 16-byte aligned" % (name, n))
            return ptrs

        m = int(sigmas.shape[0]) if isinstance(sigmas, torch.Tensor) and sigmas.dim() else len(sigmas)
        if m < 1:
            raise ValueError("sigmas: at least one column")
        s_chunks = (m + chunk - 1) // chunk
        if column_rows is None:
            rows = [u] * (k * m)
        else:
            rows = [int(r) for r in column_rows]
            if len(rows) != k * m or any(r < 0 or r > u for r in rows):
                raise ValueError("column_rows: %d values between 0 and usable_rows" % (k * m))
        sig = pointers("sigmas", sigmas, (m,), u)
        cols = pointers("columns", columns, (k, m), max(rows))
        if out is None:
            out = torch.zeros((k, s_chunks, u + 1, 4), dtype=torch.uint64, device=dev)
        elif not isinstance(out, torch.Tensor):
            raise ValueError("out must be a uint64 tensor on %s" % (dev,))
        zs = pointers("out", out, (k, s_chunks), u + 1)

        def elements(name, v, n):
            if v is None:
                raise ValueError("%s: %d field element(s)" % (name, n))
            if isinstance(v, torch.Tensor):
                v = v.cpu().numpy()
            if isinstance(v, np.ndarray):
                buf = np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 4) if v.size == 4 * n else np.zeros((0, 4), dtype=np.uint64)
            else:
                v = [v] if isinstance(v, int) else list(v)
                buf = np.array([[(int(x) >> (64 * i)) & (2**64 - 1) for i in range(4)] for x in v], dtype=np.uint64).reshape(-1, 4)
            if buf.shape != (n, 4):
                raise ValueError("%s: %d field element(s) of 4 x uint64" % (name, n))
            return buf

        b_buf, g_buf = elements("betas", betas, k), elements("gammas", gammas, k)
        o_buf, d_buf = elements("omega", omega, 1), elements("delta", delta, 1)
        status = np.zeros(k, dtype=np.uint32)
        args = N.PermutationProduct(0, chunk, u, m, (C.c_void_p * (k * m))(*cols), (C.c_uint64 * (k * m))(*rows), (C.c_void_p * m)(*sig),
                                    (C.c_void_p * (k * s_chunks))(*zs), b_buf.ctypes.data, g_buf.ctypes.data, o_buf.ctypes.data,
                                    d_buf.ctypes.data, status.ctypes.data_as(C.POINTER(C.c_uint32)))
        rep = N.PermutationReport()
        torch.cuda.synchronize(dev)                        # the tensors were made on torch's stream, the call runs on the engine's
        self._ok(self.lib.hsw_gadget_permutation_product(self.h, C.byref(args), C.byref(rep)))
        return out, status, {f[0]: getattr(rep, f[0]) for f in N.PermutationReport._fields_ if f[0] != "reserved_"}

    def ntt(self, log_n, omega, columns, out=None, input_rows=None, shift=None, scale=None, shift_after=False, pass_log=0):
        """hsw_gadget_ntt: the Fr NTT of size N = 2^log_n of device columns, natural order in and out:
        out[i] = scale * sum_j a[j] shift^j omega^(i j), or with shift_after scale * shift^i * sum_j a[j] omega^(i j).
        Returns (out, status, report): a uint64 device tensor (columns, N, 4), the uint32 numpy status array
        (HSW_NTT_CELL_NOT_BELOW_P per column: that column was not written) and the report as a dict.  columns: a
        contiguous uint64 tensor (columns, rows, 4) on the engine's device or a sequence of device addresses (ints,
        16-byte aligned).  input_rows: per column, the rows that are read (the rest count as 0); None: all N.  omega,
        shift, scale: one field element each AS STORED, as permutation_product takes its omega; shift, scale None: 1.
        halo2's lagrange_to_coeff: omega^-1, scale 1/n; coeff_to_extended: omega_ext, shift zeta, input_rows n;
        extended_to_coeff: omega_ext^-1, scale 1/N, shift 1/zeta, shift_after.  out: the caller's own contiguous uint64
        tensor (columns, rows >= N, 4) -- `columns` itself transforms in place -- or a sequence of device addresses
        (then None is returned in its place); rows beyond N are never written.  pass_log: 0, or the most points
        (log2, 1 .. 10) a launch transforms at a time."""
        import numpy as np
        import torch
        dev = self.engine.device
        log_n, pass_log = int(log_n), int(pass_log)
        if log_n < 1 or log_n > 28:
            raise ValueError("log_n must be 1 .. 28")
        if pass_log < 0 or pass_log > 10:
            raise ValueError("pass_log must be 0 .. 10")
        n_rows = 1 << log_n
        n = int(columns.shape[0]) if isinstance(columns, torch.Tensor) and columns.dim() else len(columns)
        if n < 1:
            raise ValueError("columns: at least one")
        if input_rows is None:
            rows = [n_rows] * n
        else:
            rows = [int(r) for r in input_rows]
            if len(rows) != n or any(r < 0 or r > n_rows for r in rows):
                raise ValueError("input_rows: %d values between 0 and 2^log_n" % n)

        def pointers(name, t, need):
            if isinstance(t, torch.Tensor):
                if t.dtype != torch.uint64 or t.device != dev:
                    raise ValueError("%s must be a uint64 tensor on %s" % (name, dev))
                if t.dim() != 3 or t.shape[0] != n or t.shape[1] < need or t.shape[2] != 4 or not t.is_contiguous():
                    raise ValueError("%s must be contiguous, of shape (%d, rows >= %d, 4)" % (name, n, need))
                return [t.data_ptr() + a * t.shape[1] * 32 for a in range(n)]
            ptrs = [int(p) for p in t]
            if len(ptrs) != n or any(p == 0 or p % 16 for p in ptrs):
                raise ValueError("%s: %d device addresses, 16-byte aligned" % (name, n))
            return ptrs

        ins = pointers("columns", columns, max(rows))
        if out is None:
            out = torch.zeros((n, n_rows, 4), dtype=torch.uint64, device=dev)
        outs = pointers("out", out, n_rows)

        def element(name, v, required):
            if v is None:
                if required:
                    raise ValueError("%s: one field element" % name)
                return None
            if isinstance(v, torch.Tensor):
                v = v.cpu().numpy()
            if isinstance(v, np.ndarray):
                buf = np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 4) if v.size == 4 else np.zeros((0, 4), dtype=np.uint64)
            else:
                v = [v] if isinstance(v, int) else list(v)
                buf = np.array([[(int(x) >> (64 * i)) & (2**64 - 1) for i in range(4)] for x in v], dtype=np.uint64).reshape(-1, 4)
            if buf.shape != (1, 4):
                raise ValueError("%s: one field element of 4 x uint64" % name)
            return buf

        o_buf, g_buf, c_buf = element("omega", omega, True), element("shift", shift, False), element("scale", scale, False)
        status = np.zeros(n, dtype=np.uint32)
        args = N.Ntt(N.HSW_NTT_SHIFT_AFTER if shift_after else 0, log_n, pass_log, 0, n, (C.c_void_p * n)(*ins), (C.c_uint64 * n)(*rows),
                     (C.c_void_p * n)(*outs), o_buf.ctypes.data, g_buf.ctypes.data if g_buf is not None else None,
                     c_buf.ctypes.data if c_buf is not None else None, status.ctypes.data_as(C.POINTER(C.c_uint32)))
        rep = N.NttReport()
        torch.cuda.synchronize(dev)                        # the tensors were made on torch's stream, the call runs on the engine's
        self._ok(self.lib.hsw_gadget_ntt(self.h, C.byref(args), C.byref(rep)))
        return out if isinstance(out, torch.Tensor) else None, status, {f[0]: getattr(rep, f[0]) for f in N.NttReport._fields_}

    def msm(self, bases, columns, input_rows=None, window_bits=0, slice_rows=0, n_bases=None):
        """hsw_gadget_msm: the commitments of device columns, points[b] = sum_{j < input_rows[b]} a[j] * G[j] in BN254 G1.
        Returns (points, status, report): a (columns, 8) uint64 numpy array -- x then y, four words each, Montgomery form
        mod q, all zero for the identity, as a base is stored -- the uint32 numpy status array (HSW_MSM_CELL_NOT_BELOW_P:
        that column's row of `points` is left zero; HSW_MSM_BASE_NOT_BELOW_Q: every row is) and the report as a dict.
        bases: a contiguous uint64 tensor (n_bases, 8) on the engine's device, or a device address (int, 16-byte
        aligned) with n_bases.  columns: a contiguous uint64 tensor (columns, rows, 4) on the engine's device or a
        sequence of device addresses, as ntt takes them.  input_rows: per column, the rows that are read (0 .. n_bases);
        None: all n_bases.  window_bits: 0 or 1 .. 8; slice_rows: 0 or a power of two, 64 .. 2^28."""
        import numpy as np
        import torch
        dev = self.engine.device
        window_bits, slice_rows = int(window_bits), int(slice_rows)
        if window_bits < 0 or window_bits > N.HSW_MSM_MAX_WINDOW_BITS:
            raise ValueError("window_bits must be 0 .. %d" % N.HSW_MSM_MAX_WINDOW_BITS)
        if slice_rows and (slice_rows < 64 or slice_rows > 1 << 28 or slice_rows & (slice_rows - 1)):
            raise ValueError("slice_rows must be 0 or a power of two, 64 .. 2^28")
        if isinstance(bases, (tuple, list)) and len(bases) == 2:          # (address, n_bases)
            bases, n_bases = bases
        if isinstance(bases, torch.Tensor):
            if bases.dtype != torch.uint64 or bases.device != dev:
                raise ValueError("bases must be a uint64 tensor on %s" % (dev,))
            if bases.dim() != 2 or bases.shape[1] != 8 or not bases.is_contiguous():
                raise ValueError("bases must be contiguous, of shape (n_bases, 8)")
            if n_bases is not None and int(n_bases) != bases.shape[0]:
                raise ValueError("n_bases is the tensor's")
            nb, base_ptr = int(bases.shape[0]), bases.data_ptr() if bases.shape[0] else 0
        else:
            if n_bases is None:
                raise ValueError("bases given as an address need n_bases")
            nb, base_ptr = int(n_bases), int(bases)
            if base_ptr == 0 or base_ptr % 16:
                raise ValueError("bases: a device address, 16-byte aligned")
        if nb < 1 or nb > 1 << 28:
            raise ValueError("n_bases must be 1 .. 2^28")
        n = int(columns.shape[0]) if isinstance(columns, torch.Tensor) and columns.dim() else len(columns)
        if n < 1:
            raise ValueError("columns: at least one")
        if input_rows is None:
            rows = [nb] * n
        else:
            rows = [int(r) for r in input_rows]
            if len(rows) != n or any(r < 0 or r > nb for r in rows):
                raise ValueError("input_rows: %d values between 0 and n_bases" % n)
        if isinstance(columns, torch.Tensor):
            if columns.dtype != torch.uint64 or columns.device != dev:
                raise ValueError("columns must be a uint64 tensor on %s" % (dev,))
            if columns.dim() != 3 or columns.shape[1] < max(rows) or columns.shape[2] != 4 or not columns.is_contiguous():
                raise ValueError("columns must be contiguous, of shape (%d, rows >= %d, 4)" % (n, max(rows)))
            ptrs = [columns.data_ptr() + a * columns.shape[1] * 32 for a in range(n)]
        else:
            ptrs = [int(p) for p in columns]
            if any(p == 0 or p % 16 for p in ptrs):
                raise ValueError("columns: %d device addresses, 16-byte aligned" % n)
        points = np.zeros((n, 8), dtype=np.uint64)
        status = np.zeros(n, dtype=np.uint32)
        args = N.Msm(0, window_bits, slice_rows, 0, n, nb, base_ptr, (C.c_void_p * n)(*ptrs), (C.c_uint64 * n)(*rows),
                     points.ctypes.data, status.ctypes.data_as(C.POINTER(C.c_uint32)))
        rep = N.MsmReport()
        torch.cuda.synchronize(dev)                        # the tensors were made on torch's stream, the call runs on the engine's
        self._ok(self.lib.hsw_gadget_msm(self.h, C.byref(args), C.byref(rep)))
        return points, status, {f[0]: getattr(rep, f[0]) for f in N.MsmReport._fields_ if f[0] != "reserved_"}

    def _open_columns(self, rows, columns, input_rows, tile_rows):
        """What evaluate and open share: (rows, tile_rows, n, per-column heights, per-column addresses)."""
        import torch
        dev = self.engine.device
        rows, tile_rows = int(rows), int(tile_rows)
        if rows < 1 or rows > 1 << 28:
            raise ValueError("rows must be 1 .. 2^28")
        if tile_rows and (tile_rows < N.HSW_OPEN_MIN_TILE_ROWS or tile_rows > 1 << 20 or tile_rows & (tile_rows - 1)):
            raise ValueError("tile_rows must be 0 or a power of two, %d .. 2^20" % N.HSW_OPEN_MIN_TILE_ROWS)
        n = int(columns.shape[0]) if isinstance(columns, torch.Tensor) and columns.dim() else len(columns)
        if n < 1:
            raise ValueError("columns: at least one")
        if input_rows is None:
            heights = [rows] * n
        else:
            heights = [int(r) for r in input_rows]
            if len(heights) != n or any(r < 0 or r > rows for r in heights):
                raise ValueError("input_rows: %d values between 0 and rows" % n)
        if isinstance(columns, torch.Tensor):
            if columns.dtype != torch.uint64 or columns.device != dev:
                raise ValueError("columns must be a uint64 tensor on %s" % (dev,))
            if columns.dim() != 3 or columns.shape[1] < max(heights) or columns.shape[2] != 4 or not columns.is_contiguous():
                raise ValueError("columns must be contiguous, of shape (%d, rows >= %d, 4)" % (n, max(heights)))
            ptrs = [columns.data_ptr() + a * columns.shape[1] * 32 for a in range(n)]
        else:
            ptrs = [int(p) for p in columns]
            if any(p == 0 or p % 16 for p in ptrs):
                raise ValueError("columns: %d device addresses, 16-byte aligned" % n)
        return rows, tile_rows, n, heights, ptrs

    @staticmethod
    def _field_elements(name, v, n):
        """n field elements AS STORED as an (n, 4) uint64 numpy array: ints, or a tensor / array of 4 n words."""
        import numpy as np
        import torch
        if v is None:
            raise ValueError("%s: %d field element(s)" % (name, n))
        if isinstance(v, torch.Tensor):
            v = v.cpu().numpy()
        if isinstance(v, np.ndarray):
            buf = np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 4) if v.size == 4 * n else np.zeros((0, 4), dtype=np.uint64)
        else:
            v = [v] if isinstance(v, int) else list(v)
            if any(int(x) < 0 or int(x) >> 256 for x in v):
                raise ValueError("%s: field elements of 256 bits" % name)
            buf = np.array([[(int(x) >> (64 * i)) & (2**64 - 1) for i in range(4)] for x in v], dtype=np.uint64).reshape(-1, 4)
        if buf.shape != (n, 4):
            raise ValueError("%s: %d field element(s) of 4 x uint64" % (name, n))
        return buf

    def evaluate(self, rows, columns, points, queries, input_rows=None, tile_rows=0):
        """hsw_gadget_evaluate: evals[i] = sum_{j < rows} a_b[j] z_t^j for every query i = (b, t), a column index and a
        point index.  Returns (evals, status, report): a (queries, 4) uint64 numpy array AS STORED in the representation
        of the pass, the uint32 numpy status array per COLUMN (HSW_OPEN_CELL_NOT_BELOW_P: the rows of `evals` of every
        query of that column are left zero) and the report as a dict.  columns: a contiguous uint64 tensor (columns,
        rows, 4) on the engine's device or a sequence of device addresses, as ntt takes them.  points: field elements as
        stored (ints, or an array of 4 words each).  queries: a sequence of (column, point) pairs; duplicates are
        allowed, and a column is read once for all its points.  input_rows: per column, the rows that are read (the rest
        count as 0); None: all.  tile_rows: 0, or the rows of a workgroup's tile (a power of two, 256 .. 2^20)."""
        import numpy as np
        import torch
        rows, tile_rows, n, heights, ptrs = self._open_columns(rows, columns, input_rows, tile_rows)
        if isinstance(points, (np.ndarray, torch.Tensor)):
            size = int(np.prod(points.shape))
            n_points = size // 4 if size % 4 == 0 else 0
        else:
            n_points = 1 if isinstance(points, int) else len(points)
        if n_points < 1:
            raise ValueError("points: at least one field element of 4 x uint64")
        z_buf = self._field_elements("points", points, n_points)
        qs = [(int(b), int(t)) for b, t in queries]
        if not qs or any(b < 0 or b >= n or t < 0 or t >= n_points for b, t in qs):
            raise ValueError("queries: at least one (column, point) pair of indices in range")
        nq = len(qs)
        evals = np.zeros((nq, 4), dtype=np.uint64)
        status = np.zeros(n, dtype=np.uint32)
        args = N.Evaluate(0, tile_rows, rows, n, (C.c_void_p * n)(*ptrs), (C.c_uint64 * n)(*heights), n_points, z_buf.ctypes.data, nq,
                          (C.c_uint32 * nq)(*[b for b, _ in qs]), (C.c_uint32 * nq)(*[t for _, t in qs]), evals.ctypes.data,
                          status.ctypes.data_as(C.POINTER(C.c_uint32)))
        rep = N.EvaluateReport()
        torch.cuda.synchronize(self.engine.device)         # the tensors were made on torch's stream, the call runs on the engine's
        self._ok(self.lib.hsw_gadget_evaluate(self.h, C.byref(args), C.byref(rep)))
        return evals, status, {f[0]: getattr(rep, f[0]) for f in N.EvaluateReport._fields_ if f[0] != "reserved_"}

    def open(self, rows, columns, groups, points, challenges, out=None, input_rows=None, tile_rows=0):
        """hsw_gadget_open: the opening quotients of GWC.  Group g = a sequence of column indices b_0 .. b_{m-1}, folded
        as halo2 folds (acc * v + a: c = sum_i v^(m-1-i) a_{b_i}, the first column the highest power of v =
        challenges[g]) and divided by (X - z), z = points[g]: q[j] = sum_{i>j} c[i] z^(i-j-1).  Returns (quotients, evals,
        status, report): a uint64 device tensor (groups, rows, 4) whose last row is zero -- msm commits it as it lies --
        the (groups, 4) uint64 numpy array of c(z) AS STORED, the uint32 numpy status array per GROUP
        (HSW_OPEN_CELL_NOT_BELOW_P: that group's quotient and its row of `evals` were not written) and the report as a
        dict.  columns, input_rows, tile_rows: as evaluate takes them.  points, challenges: one field element per group
        as stored.  out: the caller's own contiguous uint64 tensor (groups, rows' >= rows, 4), rows beyond `rows` are
        never written, or a sequence of device addresses (then None is returned in its place)."""
        import numpy as np
        import torch
        dev = self.engine.device
        rows, tile_rows, n, heights, ptrs = self._open_columns(rows, columns, input_rows, tile_rows)
        gs = [[int(b) for b in grp] for grp in groups]
        if not gs or any(not grp or any(b < 0 or b >= n for b in grp) for grp in gs):
            raise ValueError("groups: at least one, each of at least one column index below %d" % n)
        ng = len(gs)
        z_buf, v_buf = self._field_elements("points", points, ng), self._field_elements("challenges", challenges, ng)
        if out is None:
            out = torch.zeros((ng, rows, 4), dtype=torch.uint64, device=dev)
        if isinstance(out, torch.Tensor):
            if out.dtype != torch.uint64 or out.device != dev:
                raise ValueError("out must be a uint64 tensor on %s" % (dev,))
            if out.dim() != 3 or out.shape[0] != ng or out.shape[1] < rows or out.shape[2] != 4 or not out.is_contiguous():
                raise ValueError("out must be contiguous, of shape (%d, rows >= %d, 4)" % (ng, rows))
            qs = [out.data_ptr() + a * out.shape[1] * 32 for a in range(ng)]
        else:
            qs = [int(p) for p in out]
            if len(qs) != ng or any(p == 0 or p % 16 for p in qs):
                raise ValueError("out: %d device addresses, 16-byte aligned" % ng)
        first = [0]
        for grp in gs:
            first.append(first[-1] + len(grp))
        flat = [b for grp in gs for b in grp]
        evals = np.zeros((ng, 4), dtype=np.uint64)
        status = np.zeros(ng, dtype=np.uint32)
        args = N.Open(0, tile_rows, rows, n, (C.c_void_p * n)(*ptrs), (C.c_uint64 * n)(*heights), ng, (C.c_uint64 * (ng + 1))(*first),
                      (C.c_uint32 * len(flat))(*flat), z_buf.ctypes.data, v_buf.ctypes.data, (C.c_void_p * ng)(*qs), evals.ctypes.data,
                      status.ctypes.data_as(C.POINTER(C.c_uint32)))
        rep = N.OpenReport()
        torch.cuda.synchronize(dev)                        # the tensors were made on torch's stream, the call runs on the engine's
        self._ok(self.lib.hsw_gadget_open(self.h, C.byref(args), C.byref(rep)))
        return (out if isinstance(out, torch.Tensor) else None, evals, status,
                {f[0]: getattr(rep, f[0]) for f in N.OpenReport._fields_ if not f[0].startswith("reserved")})

    def _shplonk(self, which, rows, columns, sets, points, y, v, u, h, out, input_rows, tile_rows):
        """What shplonk_quotient and shplonk_open share: the argument rules, the call, (out, status, report)."""
        import numpy as np
        import torch
        dev = self.engine.device
        rows, tile_rows, n, heights, ptrs = self._open_columns(rows, columns, input_rows, tile_rows)
        if isinstance(points, (np.ndarray, torch.Tensor)):
            size = int(np.prod(points.shape))
            n_points = size // 4 if size % 4 == 0 else 0
        else:
            n_points = 1 if isinstance(points, int) else len(points)
        if n_points < 1:
            raise ValueError("points: at least one field element of 4 x uint64")
        z_buf = self._field_elements("points", points, n_points)
        if len({row.tobytes() for row in z_buf}) != n_points:
            raise ValueError("points: the entries must differ in value")
        ss = [([int(b) for b in cols], [int(t) for t in pts]) for cols, pts in sets]
        if not ss or len(ss) > 65535:
            raise ValueError("sets: 1 .. 65535 pairs of (column indices, point indices)")
        if any(not cols or any(b < 0 or b >= n for b in cols) for cols, _ in ss):
            raise ValueError("sets: each lists at least one column index below %d" % n)
        listed = [b for cols, _ in ss for b in cols]
        if len(set(listed)) != len(listed):
            raise ValueError("sets: a column is listed once in the whole call")
        if any(not pts or len(pts) > N.HSW_SHPLONK_MAX_SET_POINTS or any(t < 0 or t >= n_points for t in pts) or len(set(pts)) != len(pts) for _, pts in ss):
            raise ValueError("sets: each lists 1 .. %d distinct point indices below %d" % (N.HSW_SHPLONK_MAX_SET_POINTS, n_points))
        if {t for _, pts in ss for t in pts} != set(range(n_points)):
            raise ValueError("points: every entry must be used by a set")
        y_buf, v_buf = self._field_elements("y", y, 1), self._field_elements("v", v, 1)
        u_buf = self._field_elements("u", u, 1) if which == "open" else None
        h_ptr = None
        if which == "open":
            if isinstance(h, torch.Tensor):
                if h.dtype != torch.uint64 or h.device != dev or h.dim() != 2 or h.shape[0] < rows or h.shape[1] != 4 or not h.is_contiguous():
                    raise ValueError("h must be a contiguous uint64 tensor on %s of shape (rows >= %d, 4)" % (dev, rows))
                h_ptr = h.data_ptr()
            else:
                h_ptr = int(h) if h is not None else 0
                if h_ptr == 0 or h_ptr % 16:
                    raise ValueError("h: a tensor or a device address, 16-byte aligned")
        if out is None:
            out = torch.zeros((rows, 4), dtype=torch.uint64, device=dev)
        if isinstance(out, torch.Tensor):
            if out.dtype != torch.uint64 or out.device != dev or out.dim() != 2 or out.shape[0] < rows or out.shape[1] != 4 or not out.is_contiguous():
                raise ValueError("out must be a contiguous uint64 tensor on %s of shape (rows >= %d, 4)" % (dev, rows))
            out_ptr = out.data_ptr()
        else:
            out_ptr = int(out)
            if out_ptr == 0 or out_ptr % 16:
                raise ValueError("out: a tensor or a device address, 16-byte aligned")
        first, pfirst = [0], [0]
        for cols, pts in ss:
            first.append(first[-1] + len(cols))
            pfirst.append(pfirst[-1] + len(pts))
        flat_p = [t for _, pts in ss for t in pts]
        ns = len(ss)
        status = np.zeros(1, dtype=np.uint32)
        args = N.Shplonk(0, tile_rows, rows, n, (C.c_void_p * n)(*ptrs), (C.c_uint64 * n)(*heights), n_points, z_buf.ctypes.data, ns,
                         (C.c_uint64 * (ns + 1))(*first), (C.c_uint32 * len(listed))(*listed), (C.c_uint64 * (ns + 1))(*pfirst),
                         (C.c_uint32 * len(flat_p))(*flat_p), y_buf.ctypes.data, v_buf.ctypes.data, u_buf.ctypes.data if u_buf is not None else None,
                         h_ptr, out_ptr, status.ctypes.data_as(C.POINTER(C.c_uint32)))
        rep = N.ShplonkReport()
        torch.cuda.synchronize(dev)                        # the tensors were made on torch's stream, the call runs on the engine's
        fn = self.lib.hsw_gadget_shplonk_open if which == "open" else self.lib.hsw_gadget_shplonk_quotient
        self._ok(fn(self.h, C.byref(args), C.byref(rep)))
        return (out if isinstance(out, torch.Tensor) else None, int(status[0]),
                {f[0]: getattr(rep, f[0]) for f in N.ShplonkReport._fields_ if not f[0].startswith("reserved")})

    def shplonk_quotient(self, rows, columns, sets, points, y, v, out=None, input_rows=None, tile_rows=0):
        """hsw_gadget_shplonk_quotient: the first polynomial of SHPLONK's multi-point opening.  sets: a sequence of
        (column indices, point indices) pairs, the rotation sets; set i folds its columns as c_i = sum_k y^k a_{b_{i,k}}
        (the first listed column gets y^0), divides by Z_i(X) = prod (X - points[t]) over its point indices, and
        h = sum_i v^i floor(c_i / Z_i) (the first set gets v^0).  Returns (h, status, report): a uint64 device tensor
        (rows, 4) that msm commits as it lies, the status word (HSW_SHPLONK_CELL_NOT_BELOW_P: a stored cell that was
        read is not below p, and h was not written) and the report as a dict.  columns, input_rows, tile_rows: as
        evaluate takes them; a column is listed once in the whole call.  points: the distinct field elements of the
        super point set as stored, each used by a set; y, v: field elements as stored.  out: the caller's own
        contiguous uint64 tensor (rows' >= rows, 4), or a device address (then None is returned in its place)."""
        return self._shplonk("quotient", rows, columns, sets, points, y, v, None, None, out, input_rows, tile_rows)

    def shplonk_open(self, rows, columns, sets, points, y, v, u, h, out=None, input_rows=None, tile_rows=0):
        """hsw_gadget_shplonk_open: the second polynomial, after h was committed and u squeezed.  With zd_i = prod (u -
        z) over the points NOT in set i, zt the product over all points: L = sum_i v^i zd_i c_i - zt h and w[j] =
        zd_0^-1 sum_{l>j} L[l] u^(l-j-1), so that (X - u) w(X) = (L(X) - L(u)) / zd_0.  h: what shplonk_quotient
        returned for the same arguments (a (rows, 4) tensor or a device address).  Returns (w, status, report) as
        shplonk_quotient does."""
        return self._shplonk("open", rows, columns, sets, points, y, v, u, h, out, input_rows, tile_rows)

    def quotient(self, log_rows, log_n, usable_rows, columns, ys, omega_ext, zeta, fixed=None, gates=(), l0=None, l_last=None,
                 l_active=None, perm_columns=(), chunk_columns=0, sigmas=None, perm_products=None, delta=None, betas=None, gammas=None,
                 lookups=(), permuted_inputs=None, permuted_tables=None, lookup_products=None, thetas=None, out=None):
        """hsw_gadget_quotient: h(X) on the extended coset for K independent proofs of one circuit -- every gate,
        permutation and lookup expression folded with y (V = V y + expr, in the order of include/hsw.h) and divided by
        the vanishing polynomial.  Returns (h, status, report): a uint64 device tensor (K, N, 4), the uint32 numpy
        status array per proof (HSW_QUOTIENT_CELL_NOT_BELOW_P: that proof's h was not written) and the report as a dict.
        Every column holds N = 2^log_n cells in extended form.  columns: a contiguous uint64 tensor (K, m, rows >= N, 4)
        on the engine's device, or K sequences of m device addresses (16-byte aligned), as ntt takes them; fixed: the
        shared columns, a tensor (F, rows, 4) or F addresses -- column index m + j.  gates: a list of gates, each a list
        of monomials (coeff, [(column, rotation), ...]) with coeff a field element AS STORED and the rotation in base
        rows.  l0, l_last, l_active: a tensor (rows, 4) or an address each, needed with a permutation or a lookup.
        perm_columns: the permutation's column indices in its order, chunk_columns at a time; sigmas: (n_perm, rows, 4) or
        addresses; perm_products: (K, S, rows, 4) or K sequences of S addresses.  lookups: a list of (input column
        indices, table column indices), folded with theta, the first listed the highest power; permuted_inputs,
        permuted_tables, lookup_products: (K, n_lookups, rows, 4) or K sequences of addresses.  ys, betas, gammas,
        thetas: K field elements as stored; omega_ext, zeta, delta: one each.  out: the caller's own contiguous uint64
        tensor (K, rows >= N, 4), rows beyond N are never written, or K device addresses (then None is returned)."""
        import numpy as np
        import torch
        dev = self.engine.device
        log_rows, log_n, u, chunk = int(log_rows), int(log_n), int(usable_rows), int(chunk_columns)
        if log_n > 28 or log_rows < 0 or not 1 <= log_n - log_rows <= N.HSW_QUOTIENT_MAX_EXTENSION:
            raise ValueError("log_n at most 28 and log_n - log_rows 1 .. %d" % N.HSW_QUOTIENT_MAX_EXTENSION)
        n, n_ext = 1 << log_rows, 1 << log_n
        if u < 1 or u >= n:
            raise ValueError("usable_rows must be 1 .. 2^log_rows - 1")

        def grid(name, t, shape):
            """the device addresses of a grid of columns of N cells, row-major: a tensor shape + (rows >= N, 4) or nested addresses"""
            count = int(np.prod(shape)) if shape else 1
            if isinstance(t, torch.Tensor):
                if t.dtype != torch.uint64 or t.device != dev:
                    raise ValueError("%s must be a uint64 tensor on %s" % (name, dev))
                if t.dim() != len(shape) + 2 or tuple(t.shape[:len(shape)]) != tuple(shape) or t.shape[-2] < n_ext or t.shape[-1] != 4 or not t.is_contiguous():
                    raise ValueError("%s must be contiguous, of shape %s + (rows >= %d, 4)" % (name, tuple(shape), n_ext))
                return [t.data_ptr() + a * t.shape[-2] * 32 for a in range(count)]
            if t is None:
                raise ValueError("%s: %d column(s)" % (name, count))
            def flatten(v):
                return [int(v)] if isinstance(v, (int, np.integer)) else [p for row in v for p in flatten(row)]
            ptrs = flatten(t)
            if len(ptrs) != count or any(p <= 0 for p in ptrs):      # (alignment: the library's refusal names the column)
                raise ValueError("%s: %d device addresses" % (name, count))
            return ptrs

        if isinstance(columns, torch.Tensor):
            if columns.dim() != 4:
                raise ValueError("columns must be of shape (K, m, rows, 4)")
            k, m = int(columns.shape[0]), int(columns.shape[1])
        else:
            columns = [list(row) for row in columns]
            k, m = len(columns), len(columns[0]) if columns else 0
        if k < 1:
            raise ValueError("columns: at least one proof")
        cols = grid("columns", columns, (k, m)) if m else []
        if fixed is None:
            n_fixed, fix = 0, []
        else:
            n_fixed = int(fixed.shape[0]) if isinstance(fixed, torch.Tensor) and fixed.dim() else len(fixed)
            fix = grid("fixed", fixed, (n_fixed,)) if n_fixed else []
        width = m + n_fixed
        # the gates
        first_term, coeffs, first_factor, f_col, f_rot = [0], [], [0], [], []
        for gate in gates:
            for coeff, factors in gate:
                factors = [(int(cj), int(r)) for cj, r in factors]
                if len(factors) > N.HSW_QUOTIENT_MAX_FACTORS:
                    raise ValueError("gates: a monomial has at most %d factors" % N.HSW_QUOTIENT_MAX_FACTORS)
                if any(cj < 0 or cj >= width for cj, _ in factors):
                    raise ValueError("gates: a column index is not below %d" % width)
                if any(abs(r) >= n for _, r in factors):
                    raise ValueError("gates: a rotation is not below 2^log_rows in size")
                coeffs.append(int(coeff))
                f_col += [cj for cj, _ in factors]
                f_rot += [r for _, r in factors]
                first_factor.append(len(f_col))
            first_term.append(len(coeffs))
        n_gates = len(first_term) - 1
        perm = [int(j) for j in perm_columns]
        lks = [([int(j) for j in ins], [int(j) for j in tabs]) for ins, tabs in lookups]
        if not n_gates and not perm and not lks:
            raise ValueError("no gate, no permutation and no lookup: nothing to fold")
        if any(j < 0 or j >= width for j in perm):
            raise ValueError("perm_columns: a column index is not below %d" % width)
        if any(j < 0 or j >= width for ins, tabs in lks for j in ins + tabs):
            raise ValueError("lookups: a column index is not below %d" % width)
        if any(not ins or not tabs for ins, tabs in lks):
            raise ValueError("lookups: at least one input and one table column each")
        fe = self._field_elements
        y_buf, w_buf, z_buf = fe("ys", ys, k), fe("omega_ext", omega_ext, 1), fe("zeta", zeta, 1)
        c_buf = fe("gates: coefficients", coeffs, len(coeffs)) if coeffs else np.zeros((0, 4), dtype=np.uint64)
        args = N.Quotient()
        args.log_rows, args.log_n, args.chunk_columns, args.usable_rows = log_rows, log_n, chunk, u
        args.n_proofs, args.n_columns, args.n_fixed = k, m, n_fixed
        keep = [y_buf, w_buf, z_buf, c_buf]                  # what the struct points into

        def u32(v):
            a = (C.c_uint32 * max(len(v), 1))(*v)
            keep.append(a)
            return a

        def table(v):
            a = (C.c_void_p * max(len(v), 1))(*v)
            keep.append(a)
            return a
        args.d_columns, args.d_fixed = table(cols), table(fix) if n_fixed else None
        args.ys, args.omega_ext, args.zeta = y_buf.ctypes.data, w_buf.ctypes.data, z_buf.ctypes.data
        if n_gates:
            rot = (C.c_int32 * max(len(f_rot), 1))(*f_rot)
            keep.append(rot)
            args.gates = N.QuotientGates(n_gates, len(coeffs), len(f_col), u32(first_term), c_buf.ctypes.data, u32(first_factor), u32(f_col), rot)
        if perm or lks:
            b_buf, g_buf = fe("betas", betas, k), fe("gammas", gammas, k)
            keep += [b_buf, g_buf]
            args.betas, args.gammas = b_buf.ctypes.data, g_buf.ctypes.data
            args.d_l0, args.d_l_last, args.d_l_active = grid("l0", l0, ())[0], grid("l_last", l_last, ())[0], grid("l_active", l_active, ())[0]
        if perm:
            if chunk < 1:
                raise ValueError("chunk_columns is at least 1")
            sets = (len(perm) + min(chunk, len(perm)) - 1) // min(chunk, len(perm))
            d_buf = fe("delta", delta, 1)
            keep.append(d_buf)
            args.n_perm_columns, args.perm_columns, args.delta = len(perm), u32(perm), d_buf.ctypes.data
            args.d_sigmas, args.d_perm_products = table(grid("sigmas", sigmas, (len(perm),))), table(grid("perm_products", perm_products, (k, sets)))
        if lks:
            t_buf = fe("thetas", thetas, k)
            keep.append(t_buf)
            fi, ft = [0], [0]
            for ins, tabs in lks:
                fi.append(fi[-1] + len(ins))
                ft.append(ft[-1] + len(tabs))
            args.lookups = N.QuotientLookups(len(lks), u32(fi), u32([j for ins, _ in lks for j in ins]), u32(ft), u32([j for _, tabs in lks for j in tabs]),
                                             table(grid("permuted_inputs", permuted_inputs, (k, len(lks)))),
                                             table(grid("permuted_tables", permuted_tables, (k, len(lks)))),
                                             table(grid("lookup_products", lookup_products, (k, len(lks)))), t_buf.ctypes.data)
        if out is None:
            out = torch.zeros((k, n_ext, 4), dtype=torch.uint64, device=dev)
        args.d_h = table(grid("out", out, (k,)))
        status = np.zeros(k, dtype=np.uint32)
        args.status = status.ctypes.data_as(C.POINTER(C.c_uint32))
        rep = N.QuotientReport()
        torch.cuda.synchronize(dev)                        # the tensors were made on torch's stream, the call runs on the engine's
        self._ok(self.lib.hsw_gadget_quotient(self.h, C.byref(args), C.byref(rep)))
        return out if isinstance(out, torch.Tensor) else None, status, {f[0]: getattr(rep, f[0]) for f in N.QuotientReport._fields_}

    def seek(self, hash_idx):
        """Continue at digest #hash_idx as if the earlier ones had been assigned (their positions
        follow from max_variable_byte_sizes alone): lets several GPUs share one circuit's digests."""
        self._resolve_pending()
        self._ok(self.lib.hsw_gadget_seek(self.h, hash_idx))
        self._n = hash_idx

    def context_region(self, h):
        """hsw_gadget_context_region: where proof h lives on the device (context-image gadgets and Context groups)."""
        r = N.ContextRegion()
        self._ok(self.lib.hsw_gadget_context_region(self.h, h, C.byref(r)))
        return r

    def cell_position(self, cell):
        c, r = C.c_uint64(), C.c_uint64()
        self._ok(self.lib.hsw_gadget_cell_position(self.h, cell, C.byref(c), C.byref(r)))
        return int(c.value), int(r.value)

    def set_repr(self, repr_flag):
        self._ok(self.lib.hsw_gadget_set_repr(self.h, repr_flag))

    def view(self):
        v = N.GadgetView()
        self._ok(self.lib.hsw_gadget_streams(self.h, C.byref(v)))
        return v

    def streams(self):
        """Copies of the streams written so far, as numpy uint64 arrays."""
        import numpy as np
        v = self.view()
        G = self.engine.G
        ncols = self.engine.ncols

        def grab(ptr, n_cells):
            a = np.zeros((n_cells, 4), dtype=np.uint64)
            self._ok(self.lib.hsw_download(self.engine.h, a.ctypes.data, ptr, n_cells * 32))
            return a

        rows = (int(v.num_limb_sum) + ncols - 1) // ncols
        if getattr(self, "_bound", None) is not None:
            return self._bound_streams(v, grab, rows)
        if (self.context_images or self.n_contexts is not None) and int(v.max_rows):   # (K, columns, max_rows, 4): one image per proof
            k = self.n_contexts if self.n_contexts is not None else len(self.max_variable_byte_sizes)
            gate = grab(v.d_gate, k * int(v.max_rows) * int(v.columns)).reshape(k, int(v.columns), int(v.max_rows), 4)
        elif self.whole_digest and int(v.max_rows):
            gate = grab(v.d_gate, int(v.max_rows) * int(v.columns)).reshape(int(v.columns), int(v.max_rows), 4)
        else:
            gate = grab(v.d_gate, int(v.gate_cells) if self.whole_digest else int(v.blocks_done) * G)
        dense = np.stack([grab(v.d_chip_dense + c * int(v.chip_col_stride) * 32, rows) for c in range(ncols)])
        spread = np.stack([grab(v.d_chip_spread + c * int(v.chip_col_stride) * 32, rows) for c in range(ncols)])
        out = dict(gate=gate, dense=dense, spread=spread, rows=rows)
        if self.whole_digest:
            out["lookup"] = grab(v.d_lookup, int(v.lookup_cells))
        return out

    def _bound_streams(self, v, grab, rows):
        """streams() of a bound gadget: the same shapes as unbound, gathered from the caller's memory at the bound
        pitches -- the rows [0, max_rows) of every image column, Lp cells of every proof's lookup column and every
        proof's chip rows (one after the other along the row axis, as the library-owned columns hold them)."""
        import numpy as np
        b = self.region_binding()
        multi = self.context_images or self.n_contexts is not None
        k = 1 if not multi else self.n_contexts if self.n_contexts is not None else len(self.max_variable_byte_sizes)
        ncols, cols, mr = self.engine.ncols, int(v.columns), int(v.max_rows)
        cp, cap = getattr(self, "_column_ptrs", None), int(b.columns_capacity)

        def column(c, j):            # columns by pointer table: the caller's own pointer of (proof c, column j)
            return cp[c * cap + j] if cp else b.d_columns + (c * int(b.context_pitch) + j * int(b.column_pitch)) * 32
        gate = np.stack([np.stack([grab(column(c, j), mr) for j in range(cols)]) for c in range(k)])
        lp = int(self.context_region(0).lookup_cells) if multi else int(v.lookup_cells)
        lks, chips = getattr(self, "_lookup_ptrs", None), getattr(self, "_chip_ptrs", None)   # by pointer table: the caller's own pointers
        lookup = np.concatenate([grab(lks[c] if lks else b.d_lookup + c * int(b.lookup_pitch) * 32, lp) for c in range(k)])
        per = rows // k if multi else rows             # chip rows of one proof (a whole number of rows each)

        def chip(base, tab):
            return np.stack([np.concatenate([grab(tab[c * ncols + j] if tab else
                                                  base + (c * int(b.chip_context_pitch) + j * int(b.chip_col_stride)) * 32, per)
                                             for c in range(k)]) for j in range(ncols)])
        return dict(gate=gate if multi else gate[0], dense=chip(b.d_chip_dense, chips and chips[0]),
                    spread=chip(b.d_chip_spread, chips and chips[1]), rows=rows, lookup=lookup)
