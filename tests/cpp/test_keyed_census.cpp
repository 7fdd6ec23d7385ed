// The key census through include/dusk_schnorr.hpp -> libdsv.so: KeySet*::census over the `PublicKey*` objects of a
// batch — most under registered keys, some under keys the set has never seen, one without a normal form (z = 0).
// The hits per registered key, the missed keys with their counts and first items, and the totals are what the batch
// was built with.  Exit code 0 = all passed.
#include <algorithm>

#include "dusk_schnorr.hpp"
#include "support.hpp"

using namespace dusk_schnorr;

constexpr size_t kKeys = 9, kRegistered = 5, kItems = 300, kCapacity = 8;

// Set: KeySet / KeySetDouble / KeySetVarGen; sk_of(rng) draws a secret key, pk_of(sk) its public key
template <class Set, class Key, class Secret, class SkOf, class PkOf>
static void census(uint64_t seed, SkOf sk_of, PkOf pk_of) {
  Rng rng(seed);
  std::vector<Key> all;
  for (size_t k = 0; k < kKeys; k++) all.push_back(pk_of(sk_of(rng)));
  // skewed use: key k about twice as often as key k + 1
  std::vector<Key> pks;
  std::vector<size_t> which;
  for (size_t i = 0; i < kItems; i++) {
    size_t k = 0;
    while (k + 1 < kKeys && rng.next() % 2) k++;
    k = (k + 3) % kKeys;  // (so that registered and unregistered keys are both among the busy ones)
    which.push_back(k);
    pks.push_back(all[k]);
  }
  // one object without a normal form
  const size_t dead = 17;
  reinterpret_cast<JubJubExtended*>(&pks[dead])->z = BlsScalar::zero();

  std::vector<uint32_t> hits(kCapacity, 0);
  std::vector<KeyCensus::Missed> missed;
  size_t missed_items = 0, distinct = 0;
  for (size_t k = 0; k < kKeys; k++) {
    uint32_t count = 0, first = 0;
    for (size_t i = kItems; i-- > 0;)
      if (which[i] == k && i != dead) count++, first = (uint32_t)i;
    distinct += count > 0;
    if (k < kRegistered) hits[k] = count;
    else if (count) missed.push_back({first, count}), missed_items += count;
  }
  std::sort(missed.begin(), missed.end(), [](const KeyCensus::Missed& a, const KeyCensus::Missed& b) {
    return a.count != b.count ? a.count > b.count : a.first_item < b.first_item;
  });
  CHECK(missed.size() >= 2 && missed_items > 0 && missed_items < kItems);

  Set keys(std::vector<Key>(all.begin(), all.begin() + kRegistered), kCapacity);
  CHECK(keys.size() == kRegistered && keys.capacity() == kCapacity);
  const KeyCensus c = keys.census(pks);
  CHECK(c.hits == hits);
  CHECK(c.missed.size() == missed.size());
  for (size_t j = 0; j < missed.size(); j++)
    CHECK(c.missed[j].first_item == missed[j].first_item && c.missed[j].count == missed[j].count);
  CHECK(c.missed_items == missed_items + 1 && c.unusable_items == 1);
  // the policy's step: the busiest missed key is admitted, and the next census counts it among the hits
  const KeyCensus::Missed top = c.missed.front();
  const uint32_t at = keys.append({pks[top.first_item]});
  CHECK(at == kRegistered);
  const KeyCensus d = keys.census(pks.data(), pks.size());
  CHECK(d.hits[at] == top.count && d.missed.size() == missed.size() - 1);
  CHECK(d.missed_items == c.missed_items - top.count && d.unusable_items == 1);
  // an empty batch, and an empty set
  const KeyCensus e = keys.census(std::vector<Key>{});
  CHECK(e.hits == std::vector<uint32_t>(kCapacity, 0) && e.missed.empty() && e.missed_items == 0);
  Set none(std::vector<Key>{});
  const KeyCensus f = none.census(pks);
  CHECK(f.hits.empty() && f.missed_items == kItems && f.unusable_items == 1 && f.missed.size() == distinct);
}

int main() {
  census<KeySet, PublicKey, SecretKey>(
      3321, [](Rng& r) { return SecretKey::random(r); }, [](const SecretKey& sk) { return PublicKey::from(sk); });
  census<KeySetDouble, PublicKeyDouble, SecretKey>(
      3322, [](Rng& r) { return SecretKey::random(r); }, [](const SecretKey& sk) { return PublicKeyDouble::from(sk); });
  census<KeySetVarGen, PublicKeyVarGen, SecretKeyVarGen>(
      3323, [](Rng& r) { return SecretKeyVarGen::random(r); },
      [](const SecretKeyVarGen& sk) { return PublicKeyVarGen::from(sk); });
  std::printf("ok: the census of %zu items under %zu keys, %zu registered, per scheme\n", kItems, kKeys, kRegistered);
  return 0;
}
