//! The candidates of the user's `for` loop, packed once (length-bucketed tiles of 64, rfgpu.h "corpus") and kept in HBM.
use crate::metric::{check, Error};
use crate::sys::*;
use std::ffi::CString;

pub struct Corpus(pub(crate) *mut RfCorpus);
// handles are immutable after creation and may be shared between threads (rfgpu.h "Threading")
unsafe impl Send for Corpus {}
unsafe impl Sync for Corpus {}

impl Corpus {
    /// Byte candidates (`u8` elements, the reference's `HashableChar` case `u8`, details/common.rs:34).
    pub fn new<'a, I: IntoIterator<Item = &'a [u8]>>(candidates: I, device: i32) -> Result<Self, Error> {
        let (mut bytes, mut offsets) = (Vec::new(), vec![0u64]);
        for c in candidates {
            bytes.extend_from_slice(c);
            offsets.push(bytes.len() as u64);
        }
        let mut h = std::ptr::null_mut();
        check(unsafe { rf_corpus_pack(bytes.as_ptr(), offsets.as_ptr(), offsets.len() - 1, device, &mut h) })?;
        Ok(Corpus(h))
    }
    /// Entries of a slot-ordered result vector (`RF_FLAG_SLOT_ORDER`): `len()` for a single-length corpus, 64 per tile otherwise.
    pub fn slot_count(&self) -> usize {
        unsafe { rf_corpus_slot_count(self.0) }
    }
    /// The original candidate index of every slot (`u32::MAX`: the slot holds no candidate): kept once by a caller that takes its results in slot order.
    pub fn slot_index(&self) -> Result<Vec<u32>, Error> {
        let mut out = vec![0u32; self.slot_count()];
        check(unsafe { rf_corpus_slot_index(self.0, out.as_mut_ptr(), RF_MEM_HOST) })?;
        Ok(out)
    }
    /// `&str` candidates compared as `char`s (`BatchComparator::new(s.chars())`): one u32 per char, the corpus keeps its
    /// own alphabet.
    pub fn from_chars<'a, I: IntoIterator<Item = &'a str>>(candidates: I, device: i32) -> Result<Self, Error> {
        let (mut elems, mut offsets) = (Vec::<u32>::new(), vec![0u64]);
        for c in candidates {
            elems.extend(c.chars().map(|ch| ch as u32));
            offsets.push(elems.len() as u64);
        }
        let mut h = std::ptr::null_mut();
        check(unsafe { rf_corpus_pack_u32(elems.as_ptr(), offsets.as_ptr(), offsets.len() - 1, device, &mut h) })?;
        Ok(Corpus(h))
    }
    /// Ragged byte candidates already in device memory: candidate i = `d_bytes[d_offsets[i] .. d_offsets[i + 1])`, `n + 1` offsets on the same device, `n_elems`
    /// bytes readable at `d_bytes`; the call orders itself after `stream` and is synchronous (rfgpu.h rf_corpus_pack_device).
    ///
    /// # Safety
    /// `d_bytes` and `d_offsets` must be device allocations of at least `n_elems` bytes and `n + 1` offsets on `device`.
    pub unsafe fn from_device_ragged(d_bytes: *const u8, n_elems: u64, d_offsets: *const u64, n: usize, device: i32, stream: *mut std::ffi::c_void) -> Result<Self, Error> {
        let mut h = std::ptr::null_mut();
        check(rf_corpus_pack_device(d_bytes, n_elems, d_offsets, n, device, stream, &mut h))?;
        Ok(Corpus(h))
    }
    /// The same over `char`s held as u32 elements in device memory (rfgpu.h rf_corpus_pack_u32_device): the corpus [`Corpus::from_chars`] builds on the host.
    ///
    /// # Safety
    /// As [`Corpus::from_device_ragged`], with `n_elems` u32 elements readable at `d_elems`.
    pub unsafe fn from_device_chars(d_elems: *const u32, n_elems: u64, d_offsets: *const u64, n: usize, device: i32, stream: *mut std::ffi::c_void) -> Result<Self, Error> {
        let mut h = std::ptr::null_mut();
        check(rf_corpus_pack_u32_device(d_elems, n_elems, d_offsets, n, device, stream, &mut h))?;
        Ok(Corpus(h))
    }
    /// A packed corpus written by [`Corpus::save`]; validated on load.
    pub fn load(path: &str, device: i32) -> Result<Self, Error> {
        let p = CString::new(path).map_err(|_| Error(RF_ERR_INVALID_ARG, "path contains NUL".into()))?;
        let mut h = std::ptr::null_mut();
        check(unsafe { rf_corpus_load(p.as_ptr(), device, &mut h) })?;
        Ok(Corpus(h))
    }
    pub fn save(&self, path: &str) -> Result<(), Error> {
        let p = CString::new(path).map_err(|_| Error(RF_ERR_INVALID_ARG, "path contains NUL".into()))?;
        check(unsafe { rf_corpus_save(self.0, p.as_ptr()) })
    }
    /// Packed over `char`s ([`Corpus::from_chars`], or a file saved from such a corpus): read with [`Corpus::take_chars`].
    pub fn is_wide(&self) -> bool {
        unsafe { rf_corpus_is_wide(self.0) != 0 }
    }
    /// Lengths, in elements, of the candidates `indices[j] - index_base`.
    pub fn lengths(&self, indices: &[u64], index_base: u64) -> Result<Vec<u32>, Error> {
        let mut out = vec![0u32; indices.len()];
        if !indices.is_empty() {
            check(unsafe { rf_corpus_lengths(self.0, indices.as_ptr(), indices.len(), index_base, out.as_mut_ptr(), std::ptr::null_mut()) })?;
        }
        Ok(out)
    }
    /// The candidates behind the indices a top-k / filter call returned -- the `c` of `for c in corpus` -- read back out of the packed
    /// form: row `j` is candidate `indices[j] - index_base` (any order, repeats allowed).  Byte corpora only.
    pub fn take(&self, indices: &[u64], index_base: u64) -> Result<Vec<Vec<u8>>, Error> {
        if indices.is_empty() {
            return Ok(Vec::new()); // (a NULL list means "every candidate" in the C ABI)
        }
        let mut offsets = vec![0u64; indices.len() + 1];
        let (h, idx, m) = (self.0, indices.as_ptr(), indices.len());
        check(unsafe { rf_corpus_take(h, idx, m, index_base, std::ptr::null_mut(), 0, offsets.as_mut_ptr(), RF_MEM_HOST, std::ptr::null_mut()) })?;
        let mut data = vec![0u8; offsets[m] as usize];
        if !data.is_empty() {
            check(unsafe { rf_corpus_take(h, idx, m, index_base, data.as_mut_ptr(), data.len() as u64, offsets.as_mut_ptr(), RF_MEM_HOST, std::ptr::null_mut()) })?;
        }
        Ok((0..m).map(|j| data[offsets[j] as usize..offsets[j + 1] as usize].to_vec()).collect())
    }
    /// All pairs (row of `queries`, candidate of `self`) within the cutoff `args` carries (rf_join_u32): triples (query_base + row, index_base + candidate,
    /// score), ascending by (position in `query_indices`, candidate).  `metric`: `RF_LEVENSHTEIN`, `RF_INDEL`, ... ; `op`: `RF_OP_DISTANCE` or
    /// `RF_OP_SIMILARITY`; `query_indices`: the rows to join (any order, repeats allowed), `None` = every row; `upper`: keep a pair only if candidate >
    /// row -- a self-join (`queries` is `self`) then reports each unordered pair once.  A pure count first, then one call with room for everything.
    #[allow(clippy::too_many_arguments)]
    pub fn join(&self, queries: &Corpus, metric: std::os::raw::c_int, op: std::os::raw::c_int, args: &RfArgs, query_indices: Option<&[u64]>, upper: bool, query_base: u64,
                index_base: u64) -> Result<Vec<(u64, u64, usize)>, Error> {
        let (qi, m) = match query_indices {
            Some(v) if v.is_empty() => return Ok(Vec::new()),
            Some(v) => (v.as_ptr(), v.len() as u64),
            None => (std::ptr::null(), queries.len() as u64),
        };
        let flags = if upper { RF_JOIN_UPPER } else { 0 };
        let null = std::ptr::null_mut();
        let mut n = 0u64;
        check(unsafe { rf_join_u32(metric, queries.0, qi, m, self.0, op, args, flags, query_base, index_base, 0, null, null, std::ptr::null_mut(), &mut n, RF_JOIN_BY_QUERY, std::ptr::null_mut()) })?;
        let cap = n as usize;
        if cap == 0 {
            return Ok(Vec::new());
        }
        let (mut q, mut idx, mut val) = (vec![0u64; cap], vec![0u64; cap], vec![0u32; cap]);
        check(unsafe {
            rf_join_u32(metric, queries.0, qi, m, self.0, op, args, flags, query_base, index_base, n, q.as_mut_ptr(), idx.as_mut_ptr(), val.as_mut_ptr(), &mut n, RF_JOIN_BY_QUERY, std::ptr::null_mut())
        })?;
        let have = (n as usize).min(cap);
        Ok((0..have).map(|t| (q[t], idx[t], val[t] as usize)).collect())
    }
    /// `join` by f64 score (rf_join_f64): `op` is `RF_OP_NORMALIZED_DISTANCE` / `RF_OP_NORMALIZED_SIMILARITY` of a usize metric, a similarity op of
    /// `RF_FUZZ_RATIO`, or any op of `RF_JARO` / `RF_JARO_WINKLER`; `args.cutoff_f64` carries the cutoff.  The scores are the doubles the single-query
    /// filter reports, bit for bit.
    #[allow(clippy::too_many_arguments)]
    pub fn join_f64(&self, queries: &Corpus, metric: std::os::raw::c_int, op: std::os::raw::c_int, args: &RfArgs, query_indices: Option<&[u64]>, upper: bool, query_base: u64,
                    index_base: u64) -> Result<Vec<(u64, u64, f64)>, Error> {
        let (qi, m) = match query_indices {
            Some(v) if v.is_empty() => return Ok(Vec::new()),
            Some(v) => (v.as_ptr(), v.len() as u64),
            None => (std::ptr::null(), queries.len() as u64),
        };
        let flags = if upper { RF_JOIN_UPPER } else { 0 };
        let null = std::ptr::null_mut();
        let mut n = 0u64;
        check(unsafe { rf_join_f64(metric, queries.0, qi, m, self.0, op, args, flags, query_base, index_base, 0, null, null, std::ptr::null_mut(), &mut n, RF_JOIN_BY_QUERY, std::ptr::null_mut()) })?;
        let cap = n as usize;
        if cap == 0 {
            return Ok(Vec::new());
        }
        let (mut q, mut idx, mut val) = (vec![0u64; cap], vec![0u64; cap], vec![0f64; cap]);
        check(unsafe {
            rf_join_f64(metric, queries.0, qi, m, self.0, op, args, flags, query_base, index_base, n, q.as_mut_ptr(), idx.as_mut_ptr(), val.as_mut_ptr(), &mut n, RF_JOIN_BY_QUERY, std::ptr::null_mut())
        })?;
        let have = (n as usize).min(cap);
        Ok((0..have).map(|t| (q[t], idx[t], val[t])).collect())
    }
    /// The k best candidates of `self` for every row of `queries` (rf_join_topk_u32): row j holds the (index_base + candidate, score) pairs of row
    /// `query_indices[j]` (`None` = every row), best first by (score, candidate) -- ascending scores for `RF_OP_DISTANCE`, descending for `RF_OP_SIMILARITY` -- at
    /// most `k` of them.  `args` may carry a cutoff and need not.  `no_self`: a row is never offered the candidate with its own row index, so a self-join
    /// (`queries` is `self`) returns each record's k nearest other records.
    #[allow(clippy::too_many_arguments)]
    pub fn join_topk(&self, queries: &Corpus, metric: std::os::raw::c_int, op: std::os::raw::c_int, args: &RfArgs, k: u32, query_indices: Option<&[u64]>, no_self: bool,
                     index_base: u64) -> Result<Vec<Vec<(u64, usize)>>, Error> {
        let (qi, m) = match query_indices {
            Some(v) if v.is_empty() => return Ok(Vec::new()),
            Some(v) => (v.as_ptr(), v.len()),
            None => (std::ptr::null(), queries.len()),
        };
        let flags = if no_self { RF_JOIN_NO_SELF } else { 0 };
        let kk = k as usize;
        let (mut score, mut idx, mut count) = (vec![0u32; m * kk], vec![0u64; m * kk], vec![0u32; m]);
        check(unsafe {
            rf_join_topk_u32(metric, queries.0, qi, m as u64, self.0, op, args, flags, k, index_base, score.as_mut_ptr(), idx.as_mut_ptr(), count.as_mut_ptr(), std::ptr::null_mut())
        })?;
        Ok((0..m).map(|j| (0..count[j] as usize).map(|t| (idx[j * kk + t], score[j * kk + t] as usize)).collect()).collect())
    }
    /// `join_topk` by f64 score (rf_join_topk_f64): `op` is `RF_OP_NORMALIZED_DISTANCE` / `RF_OP_NORMALIZED_SIMILARITY` of the usize metrics, one of the two
    /// similarity ops of `RF_FUZZ_RATIO`, or any op of jaro / jaro_winkler; row j holds exactly the doubles, in the (score, candidate) order, that `rf_topk_f64`
    /// of a comparator over that row returns.  "Each record's best match by ratio": over a ragged corpus this ranking differs from `join_topk`'s.
    #[allow(clippy::too_many_arguments)]
    pub fn join_topk_f64(&self, queries: &Corpus, metric: std::os::raw::c_int, op: std::os::raw::c_int, args: &RfArgs, k: u32, query_indices: Option<&[u64]>, no_self: bool,
                         index_base: u64) -> Result<Vec<Vec<(u64, f64)>>, Error> {
        let (qi, m) = match query_indices {
            Some(v) if v.is_empty() => return Ok(Vec::new()),
            Some(v) => (v.as_ptr(), v.len()),
            None => (std::ptr::null(), queries.len()),
        };
        let flags = if no_self { RF_JOIN_NO_SELF } else { 0 };
        let kk = k as usize;
        let (mut score, mut idx, mut count) = (vec![0f64; m * kk], vec![0u64; m * kk], vec![0u32; m]);
        check(unsafe {
            rf_join_topk_f64(metric, queries.0, qi, m as u64, self.0, op, args, flags, k, index_base, score.as_mut_ptr(), idx.as_mut_ptr(), count.as_mut_ptr(), std::ptr::null_mut())
        })?;
        Ok((0..m).map(|j| (0..count[j] as usize).map(|t| (idx[j * kk + t], score[j * kk + t])).collect()).collect())
    }
    /// The same as `String`s, for a corpus of `char`s (a byte corpus reads as Latin-1: its bytes are the code points 0..255).
    pub fn take_chars(&self, indices: &[u64], index_base: u64) -> Result<Vec<String>, Error> {
        if indices.is_empty() {
            return Ok(Vec::new());
        }
        let mut offsets = vec![0u64; indices.len() + 1];
        let (h, idx, m) = (self.0, indices.as_ptr(), indices.len());
        check(unsafe { rf_corpus_take_u32(h, idx, m, index_base, std::ptr::null_mut(), 0, offsets.as_mut_ptr(), RF_MEM_HOST, std::ptr::null_mut()) })?;
        let mut data = vec![0u32; offsets[m] as usize];
        if !data.is_empty() {
            check(unsafe { rf_corpus_take_u32(h, idx, m, index_base, data.as_mut_ptr(), data.len() as u64, offsets.as_mut_ptr(), RF_MEM_HOST, std::ptr::null_mut()) })?;
        }
        Ok((0..m).map(|j| data[offsets[j] as usize..offsets[j + 1] as usize].iter().map(|&u| char::from_u32(u).unwrap_or(char::REPLACEMENT_CHARACTER)).collect()).collect())
    }
    pub fn len(&self) -> usize {
        unsafe { rf_corpus_count(self.0) }
    }
    pub fn is_empty(&self) -> bool {
        self.len() == 0
    }
    pub fn device(&self) -> i32 {
        unsafe { rf_corpus_device(self.0) }
    }
}
impl Drop for Corpus {
    fn drop(&mut self) {
        unsafe { rf_corpus_free(self.0) }
    }
}
