// Addition beside core/src/object/cas.rs and validation/hash.rs: cas_id and checksum of files
// whose bytes the caller has already read, from one upload of those bytes (libsdcas
// sd_fingerprints; the CPU path when the node has no gfx950 device).
//
// For the watcher's inner_update_file (core/src/location/manager/watcher/utils.rs): it
// computes FileMetadata::new -> generate_cas_id (:393) and, when the row already carries an
// integrity checksum, file_checksum on the same path a few lines later (:438-446) -- two reads
// of one file.  A caller that holds the bytes and knows the file holds exactly that many gets
// both from one pass; a caller whose metadata size may disagree with the file keeps the path
// entries of cas.rs / hash.rs, which read with the reference's semantics.
use tokio::{io, task::spawn_blocking};

/// One (cas_id, checksum) per range of `data`; ranges are (offset, len) with 16-byte aligned
/// offsets.  Empty ranges are hashed: apply FileMetadata::new's skip of empty files
/// (file_identifier/mod.rs:80-88) before storing a cas_id.
pub async fn fingerprints(data: Vec<u8>, ranges: Vec<(u64, u64)>) -> Result<Vec<(String, String)>, io::Error> {
    spawn_blocking(move || sd_cas_sys::fingerprints_blocking(&data, &ranges))
        .await
        .map_err(|e| io::Error::new(io::ErrorKind::Other, e))?
}

// inner_update_file, where it has read the file once (the bytes in `content`, fs_metadata.len()
// == content.len() checked by the caller) and the row already has an integrity checksum:
//
//     let (cas_id, checksum) = fingerprints(content, vec![(0, len)]).await
//         .map_err(|e| FileIOError::from((full_path, e)))?
//         .pop()
//         .expect("one range, one result");
//     let cas_id = (len != 0).then_some(cas_id);          // FileMetadata::new: None for an empty file
//     // ... cas_id goes where :393's did, Some(checksum) where :438-446's did.
