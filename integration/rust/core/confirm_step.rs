// New excerpt beside core/src/object/validation/: the confirm step of the duplicates view.
//
// A duplicate group of the Object index (sd_object_index_duplicate_entries: the entries of every
// cas_id with more than one link) is a candidate set: a cas_id samples files over 100 KiB
// (core/src/object/cas.rs:30-58), so equal cas_ids mean equal size, head, samples and tail, not
// equal bytes.  Before anything is merged or deleted, the group's files are hashed in full with
// ONE file_checksums call (integration/rust/core/hash.rs -> sd_file_checksums; validation/
// hash.rs:10-24 per file) and sd_cpu_dedup_confirm splits every group into classes of equal
// checksums.  The checksums arrive on the host, so this half needs no device; a caller that
// already holds cas hashes and checksums on the device (sd_fingerprint_batch_run) calls
// sd_dedup_confirm on them instead, with the same outputs.
use std::path::PathBuf;

use sd_cas_sys::{
    sd_cpu_dedup_confirm, SD_CONFIRM_CONFIRMED, SD_CONFIRM_INVALID, SD_CONFIRM_REFUTED, SD_OK,
};

use crate::{
    library::Library,
    location::file_path_helper::{file_path_for_object_validator, IsolatedFilePathData},
    prisma::file_path,
};

use super::hash::file_checksums;

/// One candidate file: its file_path row, the cas key of its group (the cas_id's 16 hex digits
/// read as a number, as the index's entries carry it) and where it is.
pub struct Candidate {
    pub file_path: file_path_for_object_validator::Data,
    pub cas_key: u64,
    pub full_path: PathBuf,
}

/// What the confirm step found for the candidates, in their order.
pub struct Confirmed {
    /// SD_CONFIRM_*: INVALID (unreadable: left alone), SINGLE, CONFIRMED, REFUTED
    pub verdict: Vec<u8>,
    /// the first candidate with the same cas_id AND the same bytes (u64::MAX when INVALID)
    pub rep: Vec<u64>,
    /// (cas key, representative, members) per confirmed set, ascending by (cas key, checksum)
    pub sets: Vec<[u64; 3]>,
    /// sd_dedup_confirm's stats: [7] counts the cas_ids that lied
    pub stats: [u64; 8],
}

/// The candidates of the duplicate entries `(cas key, Object id)`: every file_path linked to one
/// of those Objects, joined with its location's path.  (The index knows no paths; the DB does.)
pub async fn candidates_of(library: &Library, entries: &[(u64, i32)]) -> Result<Vec<Candidate>, prisma_client_rust::QueryError> {
    let Library { db, .. } = library;
    let object_ids = entries.iter().map(|(_, id)| *id).collect::<Vec<_>>();
    let rows = db
        .file_path()
        .find_many(vec![file_path::object_id::in_vec(object_ids)])
        .select(file_path_for_object_validator::select())
        .exec()
        .await?;
    Ok(rows
        .into_iter()
        .filter_map(|fp| {
            let key = u64::from_str_radix(fp.cas_id.as_deref()?, 16).ok()?;
            let location = fp.location.as_ref()?;
            let full_path = PathBuf::from(location.path.as_deref()?)
                .join(IsolatedFilePathData::try_from((location.id, &fp)).ok()?);
            Some(Candidate { file_path: fp, cas_key: key, full_path })
        })
        .collect())
}

pub async fn confirm_step(candidates: &[Candidate]) -> Result<Confirmed, std::io::Error> {
    let m = candidates.len();
    let checksums = file_checksums(candidates.iter().map(|c| c.full_path.clone()).collect()).await;

    // a file whose checksum failed is invalid: never a representative, never counted
    let keys = candidates.iter().map(|c| c.cas_key).collect::<Vec<u64>>();
    let mut hash32 = vec![0u8; 32 * m];
    let mut valid = vec![0u8; m];
    for (i, checksum) in checksums.iter().enumerate() {
        if let Ok(hex) = checksum {
            for (b, pair) in hash32[32 * i..32 * i + 32].iter_mut().zip(hex.as_bytes().chunks(2)) {
                *b = u8::from_str_radix(std::str::from_utf8(pair).unwrap_or("00"), 16).unwrap_or(0);
            }
            valid[i] = 1;
        }
    }

    let mut out = Confirmed { verdict: vec![SD_CONFIRM_INVALID; m], rep: vec![u64::MAX; m], sets: vec![[0; 3]; m / 2], stats: [0; 8] };
    let mut n_sets = 0u64;
    // a class has at least two members, so m / 2 rows always hold the sets
    let rc = unsafe {
        sd_cpu_dedup_confirm(
            keys.as_ptr(), hash32.as_ptr(), valid.as_ptr(), m as u64, out.rep.as_mut_ptr(), std::ptr::null_mut(),
            out.verdict.as_mut_ptr(), out.sets.as_mut_ptr() as *mut u64, (m / 2) as u64, &mut n_sets,
            out.stats.as_mut_ptr(),
        )
    };
    if rc != SD_OK {
        return Err(std::io::Error::new(std::io::ErrorKind::Other, sd_cas_sys::last_error()));
    }
    out.sets.truncate(n_sets as usize);
    debug_assert!(out.verdict.iter().filter(|v| **v == SD_CONFIRM_CONFIRMED).count() as u64 == out.stats[5]);
    debug_assert!(out.verdict.iter().filter(|v| **v == SD_CONFIRM_REFUTED).count() as u64 == out.stats[6]);
    // Only CONFIRMED files are safe to merge into `rep`'s Object or to offer for deletion; a
    // REFUTED file shares its cas_id with others and its bytes with none (a "sample twin").
    Ok(out)
}
